"""CPU checks of the track pool (str_er_track_pool_*; the contract is at str_er_pool_match): the header, the record's layout, the
exports, the binding, and the errors that need no GPU -- NULL pools, NULL contexts and negative arguments."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
FUNCS = ("str_er_track_pool_create", "str_er_track_pool_destroy", "str_er_track_pool_reset", "str_er_track_pool_info", "str_er_track_pool_add",
         "str_er_track_pool_add_lattice", "str_er_track_pool_join", "str_er_track_pool_clear", "str_er_track_pool_read")
MATCH = (("entry", 0), ("cost", 4), ("second_entry", 8), ("second_cost", 12), ("free_cost", 16), ("n_tried", 20), ("n_used", 24), ("n_members", 28))


def test_header_declares_the_record_the_flag_and_the_prototypes():
    full = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert re.search(r"#define\s+STR_ER_POOL_LATTICE\s+1u", txt) and re.search(r"\}\s*str_er_pool_match;", txt)
    for name in FUNCS:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
    flat = re.sub(r"\s*\n \*\s*", " ", full)
    for words in ("the concatenation, in any order, of everything added to the slot", "An empty slot reads as a track of no members: -1, -1, -1, -1, 0, 0, 0, 0",
                  "member_cost, best_member and the members' segmentations are not pooled", "a stale pool answers STR_ER_ESTATE to everything except _reset and _destroy",
                  "A slot holds at most 65536 members"):
        assert words in flat, words
    assert flat.count("str_er_pool_match") >= 5          # the three contracts that ended at the call's boundary point to the pool


def test_record_layout_c99(tmp_path):
    src = tmp_path / "t.c"
    at = " && ".join(f"offsetof(str_er_pool_match, {f}) == {o}" for f, o in MATCH)
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n'
                   f"typedef char rec_ok[sizeof(str_er_pool_match) == 32 && sizeof(str_er_pool_match) == sizeof(str_er_track_match) && {at} ? 1 : -1];\n"
                   "typedef char fl[STR_ER_POOL_LATTICE == 1u ? 1 : -1];\n"
                   "int main(void) { rec_ok a; fl b;\n"
                   "  int (*c)(str_er_ctx *, int32_t, uint32_t, str_er_track_pool **) = str_er_track_pool_create;\n"
                   "  void (*d)(str_er_track_pool *) = str_er_track_pool_destroy;\n"
                   "  int (*g)(str_er_track_pool *, const uint8_t *, int32_t, const int32_t *, const int32_t *, int32_t, const int32_t *, const int32_t *, const int32_t *,\n"
                   "           int32_t, int32_t, const int32_t *) = str_er_track_pool_add;\n"
                   "  int (*h)(str_er_track_pool *, const str_er_run_split *, int32_t, const uint8_t *, const uint8_t *, int32_t, const int32_t *, const int32_t *, int32_t,\n"
                   "           const int32_t *, const int32_t *, const int32_t *, int32_t, int32_t, const int32_t *) = str_er_track_pool_add_lattice;\n"
                   "  int (*j)(str_er_track_pool *, int32_t, const int32_t *, int32_t) = str_er_track_pool_join;\n"
                   "  int (*r)(str_er_track_pool *, const int32_t *, int32_t, str_er_pool_match *) = str_er_track_pool_read;\n"
                   "  (void)a; (void)b; (void)c; (void)d; (void)g; (void)h; (void)j; (void)r; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_library_exports_the_symbols_and_the_kernels(S):
    L = S.load_library()
    for name in FUNCS:
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS:
        assert re.search(r"\bT\s+" + name + r"\b", out), name
    syms = subprocess.run(["nm", "-C", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for kernel in ("k_pool_add", "k_pool_state_rows", "k_pool_state_lattice", "k_pool_read", "k_pool_read_final", "k_pool_join", "k_pool_clear"):
        assert re.search(r"\b" + kernel + r"\b", syms), kernel


def test_binding_and_sources(S):
    assert S.POOL_MATCH_DTYPE.itemsize == 32 and S.POOL_LATTICE == 1
    assert [(n, S.POOL_MATCH_DTYPE.fields[n][1]) for n in S.POOL_MATCH_DTYPE.names] == list(MATCH)
    for name in ("add", "add_lattice", "join", "clear", "read", "reset", "info", "close"):
        assert callable(getattr(S.TrackPool, name)), name
    for name in ("update", "read", "resolve", "text", "reset"):
        assert callable(getattr(S.WordTracker, name)), name
    build = open(os.path.join(ROOT, "scene-text-recognition_amd", "build.py")).read()
    for src in ("track_pool_kernels.hip", "api_track_pool.cpp", "track_pool_kernels.h", "track_pool_rules.h", "track_match_device.h", "lattice_track_device.h"):
        assert '"' + src + '"' in build, src
    rules = open(os.path.join(ROOT, "scene-text-recognition_amd", "csrc", "track_pool_rules.h")).read()
    assert "hip" not in re.sub(r"//.*", "", rules).lower()          # HIP-free: the sanitized check compiles it with g++ alone


def test_errors_that_need_no_gpu(S):
    L = S.load_library()
    out, n32 = C.c_void_p(), C.c_int32()
    assert L.str_er_track_pool_create(None, 4, 0, C.byref(out)) == -1
    L.str_er_track_pool_destroy(None)                     # a NULL pool: nothing happens
    assert L.str_er_track_pool_reset(None) == -1
    assert L.str_er_track_pool_info(None, C.byref(n32), None, None, None, None, None) == -1
    assert L.str_er_track_pool_add(None, None, 0, None, None, 0, None, None, None, 0, 0, None) == -1
    assert L.str_er_track_pool_add_lattice(None, None, 0, None, None, 0, None, None, 0, None, None, None, 0, 0, None) == -1
    assert L.str_er_track_pool_join(None, 0, None, 0) == -1
    assert L.str_er_track_pool_clear(None, None, 0) == -1
    assert L.str_er_track_pool_read(None, None, 0, None) == -1
