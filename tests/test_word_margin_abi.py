"""CPU checks of the word decoder's margins (str_er_set_word_margin, str_er_word_margins; the contract is at str_er_word_margin): header,
record layout, exports, the kernel's symbol, the binding, the C++ mirror and example -- and that the output is a context setting: no
STR_ER_WANT_* define came with it and STR_ER_ABI_VERSION is still 2."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
HOST = os.path.join(ROOT, "scene-text-recognition_amd", "host")
FUNCS = ("str_er_set_word_margin", "str_er_word_margins", "str_er_word_margins_host", "str_er_result_word_margins", "str_er_result_word_row_margins",
         "str_er_result_word_row_reads", "str_er_result_word_row_alts")
RECORD = (("margin", 0), ("row", 4), ("read", 8), ("alt", 12))
# the stage flags there were before this output: it is a context setting and spends none of the remaining bits
WANTS = ("NODES", "MASKS", "LINE_CROPS", "LINE_GLYPHS", "SHAPES", "TEXT_MAP", "LINE_MAP", "STROKES", "FRAME_LINES", "LINE_LINKS", "LINE_GEOM", "LINE_WORDS", "RUN_READ",
         "WORD_MATCH", "WORD_DECODE", "RUN_SPLIT", "TRACK_READ", "LATTICE_DECODE", "LATTICE_MATCH", "LATTICE_TRACK", "TRACK_DECODE")


def test_header_declares_the_record_and_the_prototypes_and_no_flag():
    full = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert re.search(r"typedef\s+struct\s+str_er_word_margin\s*\{\s*int32_t\s+margin,\s*row;\s*int32_t\s+read,\s*alt;\s*\}\s*str_er_word_margin;", txt)
    for name in FUNCS:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
    assert re.search(r"#define\s+STR_ER_ABI_VERSION\s+2\b", txt)
    wants = set(re.findall(r"#define\s+STR_ER_WANT_(\w+)", txt))
    assert wants == set(WANTS), wants ^ set(WANTS)
    assert not re.search(r"#define\s+STR_ER_\w*MARGIN", txt)
    flat = re.sub(r"\s*\n \*\s*", " ", full)
    for words in ("G_m[a] = B[a][E]", "M_i[b] = S_i[b] + GU_i[b]", "M_i[x_i] = cost", "0 on a tie", "the smallest such x that attains it",
                  "All four fields are -1 for m = 0 and for m > 32", "-1 past m", "0xFF past m", "at most 16575", "an inserted character has no row",
                  "paths that differ only in insertions are not told apart", "no lattice decode, no tracks, no pool", "Nothing is calibrated",
                  "str_er_word_margin (str_er_set_word_margin)", "A context setting, not a stage flag"):
        assert words in flat, words


def test_record_layout_c99(tmp_path):
    src = tmp_path / "t.c"
    at = " && ".join(f"offsetof(str_er_word_margin, {f}) == {o}" for f, o in RECORD)
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n'
                   f"typedef char rec_ok[sizeof(str_er_word_margin) == 16 && {at} ? 1 : -1];\n"
                   "typedef char abi[STR_ER_ABI_VERSION == 2 ? 1 : -1];\n"
                   "int main(void) { rec_ok a; abi b;\n"
                   "  int (*f)(str_er_ctx *, int32_t) = str_er_set_word_margin;\n"
                   "  int (*g)(str_er_ctx *, const uint8_t *, int32_t, const int32_t *, const int32_t *, int32_t, str_er_word_margin *, int32_t *, uint8_t *, uint8_t *,\n"
                   "           int32_t *) = str_er_word_margins;\n"
                   "  int (*h)(const uint8_t *, int32_t, const int32_t *, const int32_t *, int32_t, const uint8_t *, int32_t, int32_t, str_er_word_margin *, int32_t *,\n"
                   "           uint8_t *, uint8_t *, int32_t *) = str_er_word_margins_host;\n"
                   "  const str_er_word_margin *(*p)(const str_er_result *, int32_t *) = str_er_result_word_margins;\n"
                   "  const int32_t *(*q)(const str_er_result *, uint64_t *) = str_er_result_word_row_margins;\n"
                   "  const uint8_t *(*s)(const str_er_result *, uint64_t *) = str_er_result_word_row_reads;\n"
                   "  const uint8_t *(*t)(const str_er_result *, uint64_t *) = str_er_result_word_row_alts;\n"
                   "  (void)a; (void)b; (void)f; (void)g; (void)h; (void)p; (void)q; (void)s; (void)t; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_library_exports_the_symbols_and_holds_the_kernel(S):
    L = S.load_library()
    assert L.str_er_abi_version() == 2
    for name in FUNCS:
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS:
        assert re.search(r"\bT\s+" + name + r"\b", out), name
    syms = subprocess.run(["nm", "-C", S.lib_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bk_word_margin\b", syms) and re.search(r"\bk_word_decode\b", syms)


def test_argument_errors_of_the_raw_entry_points(S):
    L = S.load_library()
    B, Cr = np.zeros((66, 66), np.uint8), np.zeros((3, 65), np.uint8)
    one = np.zeros(1, np.int32)
    rec, rm, rb = np.zeros(1, S.WORD_MARGIN_DTYPE), np.zeros(32, np.int32), np.zeros(32, np.uint8)
    host = L.str_er_word_margins_host
    assert host(Cr.ctypes.data, 3, one.ctypes.data, one.ctypes.data, 1, None, 0, 0, rec.ctypes.data, rm.ctypes.data, rb.ctypes.data, rb.ctypes.data, None) == -1
    assert host(Cr.ctypes.data, 3, one.ctypes.data, one.ctypes.data, 1, B.ctypes.data, 0, 0, None, rm.ctypes.data, rb.ctypes.data, rb.ctypes.data, None) == -1
    assert host(Cr.ctypes.data, 3, one.ctypes.data, one.ctypes.data, 1, B.ctypes.data, 0, 0, rec.ctypes.data, None, rb.ctypes.data, rb.ctypes.data, None) == -1
    assert host(None, 0, None, None, 0, B.ctypes.data, 0, 0, None, None, None, None, None) == 0
    assert host(Cr.ctypes.data, 3, one.ctypes.data, one.ctypes.data, 1, B.ctypes.data, 0, 0, rec.ctypes.data, rm.ctypes.data, rb.ctypes.data, rb.ctypes.data, None) == 0
    assert tuple(int(v) for v in rec[0]) == (-1, -1, -1, -1)             # (a word of no rows)
    assert L.str_er_set_word_margin(None, 1) == -1 and L.str_er_word_margins(None, None, 0, None, None, 0, None, None, None, None, None) == -1
    n = C.c_int32(7)
    assert L.str_er_result_word_margins(None, n) is None and n.value == 0
    for fn in (L.str_er_result_word_row_margins, L.str_er_result_word_row_reads, L.str_er_result_word_row_alts):
        nb = C.c_uint64(7)
        assert fn(None, nb) is None and nb.value == 0


def test_binding_dtype_methods_and_accessors(S):
    d = S.WORD_MARGIN_DTYPE
    assert d.itemsize == 16 and tuple((n, d.fields[n][1]) for n in d.names) == RECORD
    binding = __import__("importlib").import_module("scene-text-recognition_amd.binding")
    assert not [n for n in dir(binding) if n.startswith("WANT_") and "MARGIN" in n]
    for m in ("text_detect", "text_detect_list"):
        assert not [p for p in inspect.signature(getattr(S.ERFilter, m)).parameters if "margin" in p]
    assert callable(S.ERFilter.set_word_margin) and callable(S.ERFilter.word_margins) and callable(S.FrameStream.set_word_margin) and callable(S.word_margins_host)
    assert inspect.signature(S.ERFilter.word_margins).parameters["want_marginals"].default is False
    assert inspect.signature(S.word_margins_host).parameters["want_marginals"].default is False
    for m in ("word_margins", "word_row_margins", "word_row_reads", "word_row_alts"):
        assert isinstance(getattr(S.Result, m), property)
    r = S.Result.__new__(S.Result)
    r._word_margins = r._word_row_margins = r._word_row_reads = r._word_row_alts = None
    for name in ("word_margins", "word_row_margins", "word_row_reads", "word_row_alts"):
        with pytest.raises(ValueError):
            getattr(r, name)
    with pytest.raises(ValueError):
        r.word_decode_margin(0)


def test_margin_accessors_on_a_made_up_result(S):
    """word_decode_margin / word_decode_char_margins from the tables alone: a decoded word with an inserted character and a dropped run,
    and one that was not decoded."""
    r = S.Result.__new__(S.Result)
    r._words = np.zeros(2, S.LINE_WORD_DTYPE)
    r._words["first_run"], r._words["n_runs"] = [0, 3], [3, 40]
    r._word_decodes = np.zeros(2, S.WORD_DECODE_DTYPE)
    r._word_decodes["cost"], r._word_decodes["n_chars"] = [9, -1], [3, 0]
    r._word_decode_chars = np.full((2, 64), 255, np.uint8)
    r._word_decode_src = np.full((2, 64), 255, np.uint8)
    r._word_decode_chars[0, :3] = [1, 2, 3]
    r._word_decode_src[0, :3] = [0, 0x80, 2]                             # (run 1 is dropped)
    r._word_margins = np.zeros(2, S.WORD_MARGIN_DTYPE)
    r._word_margins[0] = (4, 1, 65, 7)
    r._word_margins[1] = (-1, -1, -1, -1)
    r._word_row_margins = np.full((2, 32), -1, np.int32)
    r._word_row_margins[0, :3] = [11, 4, 6]
    assert r.word_decode_margin(0) == 4 and r.word_decode_char_margins(0) == [11, -1, 6]
    assert r.word_decode_margin(1) == -1 and r.word_decode_char_margins(1) == [-1] * 40


def test_cpp_mirror_and_example_compile():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HOST, "example_word_decode.cpp")], check=True)
    txt = open(os.path.join(HOST, "er_filter_hip.hpp")).read()
    for words in ("set_word_margin", "struct WordMargins", "str_er_word_margins(", "str_er_result_word_row_alts("):
        assert words in txt, words
    assert "margin" in open(os.path.join(HOST, "example_word_decode.cpp")).read()
