"""CPU checks of the track decode (STR_ER_WANT_TRACK_DECODE; the contract is at str_er_track_decode): header, record layout, exports,
binding, the setter's ranges, the errors of the pure host entry point, the C++ mirror and example, and the verdicts of check_stages and
read_plan for the new flag -- and without it, where both answer as before."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import track_decode_ref as TD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
HOST = os.path.join(ROOT, "scene-text-recognition_amd", "host")
CSRC = os.path.join(ROOT, "scene-text-recognition_amd", "csrc")
FUNCS = ("str_er_set_track_decode", "str_er_decode_tracks", "str_er_decode_tracks_host", "str_er_result_track_decodes", "str_er_result_track_decode_chars",
         "str_er_result_track_decode_member_costs")
RECORD = (("cost", 0), ("seed_cost", 4), ("n_chars", 8), ("n_edits", 12), ("converged", 16), ("n_used", 20), ("seed_member", 24), ("lm_cost", 28))


def test_header_declares_the_flag_the_record_and_the_prototypes():
    full = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert re.search(r"#define\s+STR_ER_WANT_TRACK_DECODE\s+\(536870912u\)", txt)
    assert re.search(r"\}\s*str_er_track_decode;", txt)
    for name in FUNCS:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
    flat = re.sub(r"\s*\n \*\s*", " ", full)
    for words in ("A member is usable iff m_i <= 32", "A track has at most 1024 members", "the first 32 usable members, in slot order",
                  "The step is the neighbour with the smallest (J, index)", "a local optimum of single edits from the set median, not the global median string",
                  "a joint search over the members' piece lattices is not part of it", "Nothing is pooled across calls",
                  "Whether the polish helps on real text has not been measured", "is a separate output, str_er_track_decode",
                  "There is no pooled open-vocabulary decode across calls"):
        assert words in flat, words
    assert "(a median string over members with different run counts is another problem)" not in flat


def test_record_layout_c99(tmp_path):
    src = tmp_path / "t.c"
    at = " && ".join(f"offsetof(str_er_track_decode, {f}) == {o}" for f, o in RECORD)
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n'
                   f"typedef char rec_ok[sizeof(str_er_track_decode) == 32 && {at} ? 1 : -1];\n"
                   "typedef char fl[STR_ER_WANT_TRACK_DECODE == 536870912u && STR_ER_WANT_TRACK_DECODE == (1u << 29) && STR_ER_WANT_LATTICE_TRACK == (1u << 28) ? 1 : -1];\n"
                   "int main(void) { rec_ok a; fl b;\n"
                   "  int (*f)(str_er_ctx *, int32_t, int32_t, int32_t) = str_er_set_track_decode;\n"
                   "  int (*g)(str_er_ctx *, const uint8_t *, int32_t, const int32_t *, const int32_t *, int32_t, const int32_t *, const int32_t *, const int32_t *,\n"
                   "           int32_t, int32_t, str_er_track_decode *, uint8_t *, int32_t *) = str_er_decode_tracks;\n"
                   "  int (*h)(const uint8_t *, int32_t, const int32_t *, const int32_t *, int32_t, const int32_t *, const int32_t *, const int32_t *, int32_t, int32_t,\n"
                   "           const uint8_t *, int32_t, int32_t, int32_t, int32_t, int32_t, str_er_track_decode *, uint8_t *, int32_t *) = str_er_decode_tracks_host;\n"
                   "  const str_er_track_decode *(*p)(const str_er_result *, int32_t *) = str_er_result_track_decodes;\n"
                   "  const uint8_t *(*q)(const str_er_result *, uint64_t *) = str_er_result_track_decode_chars;\n"
                   "  const int32_t *(*r)(const str_er_result *, int32_t *) = str_er_result_track_decode_member_costs;\n"
                   "  (void)a; (void)b; (void)f; (void)g; (void)h; (void)p; (void)q; (void)r; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_library_exports_the_symbols(S):
    L = S.load_library()
    for name in FUNCS:
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS:
        assert re.search(r"\bT\s+" + name + r"\b", out), name
    syms = subprocess.run(["nm", "-C", S.lib_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bk_track_decode\b", syms)


def test_binding_constants_dtypes_and_keywords(S):
    assert S.WANT_TRACK_DECODE == 1 << 29 == 536870912
    d = S.TRACK_DECODE_DTYPE
    assert d.itemsize == 32 and tuple((n, d.fields[n][1]) for n in d.names) == RECORD and d.names == TD.DECODE_FIELDS
    for m in ("text_detect", "text_detect_list"):
        assert inspect.signature(getattr(S.ERFilter, m)).parameters["want_track_decode"].default is False
    for m in ("submit", "submit_nv12", "submit_copy", "submit_list", "submit_nv12_list", "submit_copy_list"):
        assert inspect.signature(getattr(S.FrameStream, m)).parameters["want_track_decode"].default is False
    binding = __import__("importlib").import_module("scene-text-recognition_amd.binding")
    assert binding._want_flags(track_decode=True) == 536870912 and binding._want_flags(track_read=True, track_decode=True) == 536870912 | 33554432
    assert binding._want_flags(track_read=True) == 33554432 and binding._want_flags() == 0
    for m in ("set_track_decode", "decode_tracks"):
        assert callable(getattr(S.ERFilter, m)), m
    assert callable(S.FrameStream.set_track_decode) and callable(S.decode_tracks_host)
    for m in ("track_decodes", "track_decode_chars", "track_decode_member_costs"):
        assert isinstance(getattr(S.Result, m), property)
    for m in ("word_track_decode_text", "text_track_decode_text"):
        assert callable(getattr(S.Result, m))


def test_result_accessors_without_the_flag(S):
    r = S.Result.__new__(S.Result)
    r._track_decodes = r._track_decode_chars = r._track_decode_member_costs = None
    for name in ("track_decodes", "track_decode_chars", "track_decode_member_costs"):
        with pytest.raises(ValueError):
            getattr(r, name)
    L = S.load_library()
    for name, n in ((FUNCS[3], C.c_int32(7)), (FUNCS[4], C.c_uint64(7)), (FUNCS[5], C.c_int32(7))):
        assert getattr(L, name)(None, C.byref(n)) is None and n.value == 0


def test_host_entry_point_errors_and_the_setter(S):
    L = S.load_library()
    rng = np.random.default_rng(3)
    B = rng.integers(0, 100, (66, 66)).astype(np.uint8)
    costs = rng.integers(0, 256, (3, 65)).astype(np.uint8)
    args = dict(costs=costs, first_run=[0, 2], n_runs_of_word=[2, 1], table=B)
    got, ch, mc = S.decode_tracks_host(track_first=[0], track_count=[2], members=[0, 1], **args)
    want, wch, wmc, _ = TD.decode_tracks(costs, [0, 2], [2, 1], [0], [2], np.array([0, 1]), B)
    assert TD.as_tuples(got) == want and (ch == wch).all() and mc.tolist() == wmc.tolist()
    got, ch, mc = S.decode_tracks_host(track_first=[], track_count=[], members=[], **args)
    assert got.shape == (0,) and got.dtype == S.TRACK_DECODE_DTYPE and ch.shape == (0, 32) and mc.shape == (0,)
    got, ch, mc = S.decode_tracks_host(track_first=[1], track_count=[1], members=[1, 0, 1], **args)          # slots of no track
    assert mc[0] == -1 and mc[2] == -1 and mc[1] >= 0
    for tf, tc, mem in (([0], [1], [2]), ([0], [1], [-1]), ([0], [2], [0]), ([1], [1], [0]), ([0], [-1], [0]), ([0, 0], [1, 1], [0])):
        with pytest.raises(S.StrErError) as e:
            S.decode_tracks_host(track_first=tf, track_count=tc, members=mem, **args)
        assert e.value.code == -1, (tf, tc, mem)
    with pytest.raises(S.StrErError) as e:
        S.decode_tracks_host(track_first=[0], track_count=[1025], members=np.zeros(1025, np.int32), **args)
    assert e.value.code == -7
    got, _, mc = S.decode_tracks_host(track_first=[0], track_count=[1024], members=np.zeros(1024, np.int32), rounds=0, **args)
    assert int(got[0]["n_used"]) == 1024 and int(got[0]["cost"]) == int(got[0]["lm_cost"]) + int(mc.sum())
    for kw in (dict(ins=0), dict(ins=256), dict(dele=0), dict(dele=256), dict(rounds=-1), dict(rounds=65), dict(dec_ins=-1), dict(dec_ins=256), dict(dec_dele=256)):
        with pytest.raises(S.StrErError) as e:
            S.decode_tracks_host(track_first=[0], track_count=[1], members=[0], **kw, **args)
        assert e.value.code == -1, kw
    for kw in (dict(ins=1, dele=255, rounds=0), dict(ins=255, dele=1, rounds=64), dict(dec_ins=255, dec_dele=255), dict(dec_ins=0, dec_dele=0)):
        S.decode_tracks_host(track_first=[0], track_count=[1], members=[0], **kw, **args)
    with pytest.raises(S.StrErError):
        S.decode_tracks_host(costs, [2], [2], [0], [1], [0], B)                         # a word outside the rows
    assert L.str_er_decode_tracks_host(None, 1, None, None, 0, None, None, None, 0, 0, None, 0, 0, 64, 64, 8, None, None, None) == -1
    assert L.str_er_decode_tracks_host(None, 0, None, None, 0, None, None, None, 0, 0, None, 0, 0, 64, 64, 8, None, None, None) == -1          # no table
    assert L.str_er_set_track_decode(None, 64, 64, 8) == -1
    assert L.str_er_decode_tracks(None, None, 0, None, None, 0, None, None, None, 0, 0, None, None, None) == -1


RULES_MAIN = r"""
#include "stage_rules.h"
#include "read_plan.h"
#include <cstdio>
using namespace str_er_host;
int main()
{
    const uint32_t base = STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_LINKS | STR_ER_WANT_LINE_WORDS |
                          STR_ER_WANT_RUN_READ | STR_ER_WANT_WORD_DECODE, full = base | STR_ER_WANT_TRACK_DECODE;
    const CallShape frames{true, true, false, false}, strip{false, false, true, false}, planes{false, false, false, false};
    const auto show = [](const char *what, const StageVerdict &v) { std::printf("%s|%d|%s\n", what, v.code, v.msg ? v.msg : ""); };
    show("ok", check_stages(full, frames, true, true, false, true));
    show("no_table", check_stages(full, frames, true, true, false, false));
    show("strip", check_stages(full, strip, true, true, false, true));
    show("planes", check_stages(full, planes, true, true, false, true));
    show("no_links", check_stages(full & ~STR_ER_WANT_LINE_LINKS, frames, true, true, false, true));
    show("no_decode", check_stages(full & ~STR_ER_WANT_WORD_DECODE, frames, true, true, false, true));
    show("with_match_no_lexicon", check_stages(full | STR_ER_WANT_WORD_MATCH, frames, true, true, false, true));
    show("without_flag", check_stages(base, frames, true, true, false, true));
    show("without_flag_strip", check_stages(base, strip, true, true, false, true));
    show("track_read_still_needs_match", check_stages(base | STR_ER_WANT_TRACK_READ, frames, true, true, false, true));
    const ReadPlan p = read_plan(false, true, true, false, false, false, false, false, true), q = read_plan(false, true, true, false, false, false);
    std::printf("plan|%d %d|%d %d %d %d|%d %d\n", p.tdecode, q.tdecode, p.decode_set, q.decode_set, p.parts[SET_U], q.parts[SET_U], p.result_set, q.result_set);
    const ReadPlan r = read_plan(true, false, false, false, true, true, false, false, true);
    std::printf("plan_no_decode|%d|%d\n", r.tdecode, r.track);
    return 0;
}
"""


def test_stage_verdicts_and_the_plan(tmp_path):
    src = tmp_path / "rules_main.cpp"
    src.write_text(RULES_MAIN)
    exe = str(tmp_path / "rules_main")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", exe], check=True)
    out = dict(line.split("|", 1) for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert out["ok"] == "0|"
    assert out["no_table"].startswith("-6|STR_ER_WANT_WORD_DECODE needs a bigram table")
    assert out["strip"] == "-1|STR_ER_WANT_TRACK_DECODE is not supported by the strip path (str_er_strip_merge)"
    assert out["planes"] == "-1|STR_ER_WANT_TRACK_DECODE needs frames (not the per-plane calls)"
    assert out["no_links"] == "-1|STR_ER_WANT_TRACK_DECODE needs STR_ER_WANT_LINE_LINKS"
    assert out["no_decode"] == "-1|STR_ER_WANT_TRACK_DECODE needs STR_ER_WANT_WORD_DECODE"
    assert out["with_match_no_lexicon"].startswith("-6|STR_ER_WANT_WORD_MATCH needs a lexicon")
    assert out["without_flag"] == "0|"                         # as before: the call without the flag meets no new rule
    assert out["without_flag_strip"].startswith("-1|STR_ER_WANT_WORD_DECODE is not supported by the strip path")
    assert out["track_read_still_needs_match"] == "-1|STR_ER_WANT_TRACK_READ needs STR_ER_WANT_WORD_MATCH"
    assert out["plan"] == "1 0|1 1 1 1|1 1" and out["plan_no_decode"] == "0|1"


def test_cpp_mirror_and_example_compile():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HOST, "example_track_decode.cpp")], check=True)
