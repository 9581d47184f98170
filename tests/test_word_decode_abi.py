"""CPU checks of the word decoder (STR_ER_WANT_WORD_DECODE, str_er_set_bigram, str_er_decode_words; the contract is at
str_er_word_decode): header, record layout, exports, binding, the C++ mirror and example, and the pure host entry points --
str_er_bigram_from_probs, str_er_decode_words_host -- against the reference (word_decode_ref.py), every value with ==."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import word_decode_ref as WD
import word_match_ref as WM
from test_word_decode_ref import PAIRS, insertion_vector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
HOST = os.path.join(ROOT, "scene-text-recognition_amd", "host")
FUNCS = ("str_er_set_bigram", "str_er_bigram_info", "str_er_set_word_decode", "str_er_bigram_from_probs", "str_er_decode_words", "str_er_decode_words_host",
         "str_er_result_word_decodes", "str_er_result_word_decode_chars", "str_er_result_word_decode_src")
RECORD = (("cost", 0), ("read_cost", 4), ("n_chars", 8), ("n_sub", 12), ("n_del", 16), ("n_ins", 20))


def test_header_declares_the_flag_the_record_and_the_prototypes():
    full = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert re.search(r"#define\s+STR_ER_WANT_WORD_DECODE\s+\(8388608u\)", txt)
    assert re.search(r"typedef\s+struct\s+str_er_word_decode\s*\{\s*int32_t\s+cost,\s*read_cost;\s*int32_t\s+n_chars,\s*n_sub;\s*int32_t\s+n_del,\s*n_ins;"
                     r"\s*\}\s*str_er_word_decode;", txt)
    for name in FUNCS:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
    flat = re.sub(r"\s*\n \*\s*", " ", full)
    for words in ("66 x 66 bytes, row-major", "never folded", "0 switches a move off", "INF = 2^20", "the predecessor the smallest a that attains the minimum",
                  "on a tie SUB stays", "only after some character", "(i-1) | 0x80", "padded with 0xFF past n_chars", "cost <= read_cost",
                  "A word with m > 32 is not decoded: cost = -1", "has not been checked", "str_er_word_decode (STR_ER_WANT_WORD_DECODE)",
                  "no spelling correction and no language model", "touching glyphs reads as one character"):
        assert words in flat, words


def test_record_layout_c99(tmp_path):
    src = tmp_path / "t.c"
    at = " && ".join(f"offsetof(str_er_word_decode, {f}) == {o}" for f, o in RECORD)
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n'
                   f"typedef char dec_ok[sizeof(str_er_word_decode) == 24 && {at} ? 1 : -1];\n"
                   "typedef char fl[STR_ER_WANT_WORD_DECODE == 8388608u && STR_ER_WANT_WORD_DECODE == (1u << 23) && STR_ER_WANT_WORD_MATCH == (1u << 22) ? 1 : -1];\n"
                   "int main(void) { dec_ok a; fl b;\n"
                   "  int (*f)(str_er_ctx *, const uint8_t *) = str_er_set_bigram;\n"
                   "  int (*g)(str_er_ctx *, const uint8_t *, int32_t, const int32_t *, const int32_t *, int32_t, str_er_word_decode *, uint8_t *, uint8_t *) = str_er_decode_words;\n"
                   "  int (*h)(const double *, const double *, const double *, uint8_t *) = str_er_bigram_from_probs;\n"
                   "  int (*i)(str_er_ctx *, int32_t, int32_t) = str_er_set_word_decode;\n"
                   "  int (*j)(const str_er_ctx *, int32_t *, uint64_t *) = str_er_bigram_info;\n"
                   "  int (*k)(const uint8_t *, int32_t, const int32_t *, const int32_t *, int32_t, const uint8_t *, int32_t, int32_t, str_er_word_decode *, uint8_t *,\n"
                   "           uint8_t *) = str_er_decode_words_host;\n"
                   "  const str_er_word_decode *(*p)(const str_er_result *, int32_t *) = str_er_result_word_decodes;\n"
                   "  const uint8_t *(*q)(const str_er_result *, uint64_t *) = str_er_result_word_decode_src;\n"
                   "  (void)a; (void)b; (void)f; (void)g; (void)h; (void)i; (void)j; (void)k; (void)p; (void)q; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_library_exports_the_symbols(S):
    L = S.load_library()
    for name in FUNCS:
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS:
        assert re.search(r"\bT\s+" + name + r"\b", out), name
    syms = subprocess.run(["nm", "-C", S.lib_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bk_word_decode\b", syms)


def test_bigram_from_probs_equals_cost_of_the_reference(S):
    rng = np.random.default_rng(3)
    tp = np.exp2(-rng.uniform(0, 34, (65, 65)))
    tp.reshape(-1)[:255] = WM.T                                         # every threshold, and values the contract names
    tp.reshape(-1)[255:510] = np.nextafter(WM.T, 0.0)
    tp.reshape(-1)[510:516] = [0.0, 1.0, np.nan, -1.0, np.inf, 5e-324]
    start, end = np.exp2(-rng.uniform(0, 10, 65)), np.exp2(-rng.uniform(0, 40, 65))
    got = S.bigram_from_probs(tp, start, end)
    assert got.shape == (66, 66) and got.dtype == np.uint8
    assert (got[:65, :65] == WM.cost(tp)).all() and (got[65, :65] == WM.cost(start)).all() and (got[:65, 65] == WM.cost(end)).all() and got[65, 65] == 0
    bare = S.bigram_from_probs(tp)
    assert (bare[:65, :65] == WM.cost(tp)).all() and (bare[65] == 0).all() and (bare[:, 65] == 0).all()
    L = S.load_library()
    out = np.zeros(4356, np.uint8)
    assert L.str_er_bigram_from_probs(None, None, None, out.ctypes.data) == -1 and L.str_er_bigram_from_probs(tp.ctypes.data, None, None, None) == -1


def test_bigram_from_words_and_load_tp_table(S, tmp_path):
    words = ["HOTEL", "HOT", "TO", "(A)"]
    B = S.bigram_from_words(words, alpha=1.0)
    cnt = np.ones((66, 66))
    lab = WM.LABEL_OF
    for w in words:
        seq = [65] + [lab[ch] for ch in w] + [65]
        for a, b in zip(seq, seq[1:]):
            cnt[a, b] += 1
    p = cnt / cnt.sum(axis=1, keepdims=True)
    want = WM.cost(p)
    want[65, 65] = 0
    assert (B == want).all()
    assert B[lab["H"], lab["O"]] < B[lab["H"], lab["X"]] and B[65, lab["H"]] < B[65, lab["O"]] and B[lab["L"], 65] < B[lab["L"], lab["L"]]
    with pytest.raises(ValueError):
        S.bigram_from_words(["A-B"])
    tp = np.random.default_rng(4).random((65, 65))
    path = tmp_path / "tp_table.txt"
    path.write_text("\n".join(" ".join(repr(float(v)) for v in row) for row in tp))
    assert (S.load_tp_table(str(path)) == S.bigram_from_probs(tp)).all()
    path.write_text("1 2 3")
    with pytest.raises(ValueError):
        S.load_tp_table(str(path))


def _rows(rng, n):
    c = rng.integers(60, 256, (n, 65))
    cheap = rng.random((n, 65)) < 0.08
    c[cheap] = rng.integers(0, 24, int(cheap.sum()))
    return c.astype(np.uint8)


def test_decode_words_host_equals_the_reference(S):
    rng = np.random.default_rng(11)
    n_of = np.array([0, 1, 2, 8, 9, 16, 17, 31, 32, 33] + list(rng.integers(0, 13, 20)))
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]])
    costs = _rows(rng, int(n_of.sum()))
    for ins, dele in PAIRS:
        B = rng.integers(0, 256, (66, 66)).astype(np.uint8) if ins != 1 else rng.integers(0, 3, (66, 66)).astype(np.uint8)
        want = WD.decode_words(costs, first, n_of, B, ins, dele)
        dec, chars, src = S.decode_words_host(costs, first, n_of, B, ins, dele)
        assert dec.dtype == S.WORD_DECODE_DTYPE and chars.shape == src.shape == (len(n_of), 64)
        assert WD.as_tuples(dec) == want[0], (ins, dele)
        assert (chars == want[1]).all() and (src == want[2]).all(), (ins, dele)
    # the fixed vectors
    dec, chars, src = S.decode_words_host(np.zeros((5, 65), np.uint8), [0], [5], np.zeros((66, 66), np.uint8), 64, 64)
    assert WD.as_tuples(dec) == [(0, 0, 5, 5, 0, 0)] and chars[0, :5].tolist() == [0] * 5 and src[0, :6].tolist() == [0, 1, 2, 3, 4, 255]
    Cv, Bv = insertion_vector()
    dec, chars, src = S.decode_words_host(Cv, [0], [32], Bv, 1, 0)
    assert WD.as_tuples(dec)[0][0] == 32 and chars[0].tolist() == [63, 64] * 32 and src[0].tolist() == [v for i in range(32) for v in (i, 0x80 | i)]
    full = np.full((33, 65), 255, np.uint8)
    dec, chars, src = S.decode_words_host(full, [0, 0], [32, 33], np.full((66, 66), 255, np.uint8), 255, 255)
    assert WD.as_tuples(dec) == [(33 * 255, 65 * 255, 0, 0, 32, 0), (-1, 67 * 255, 0, 0, 0, 0)] and (chars == 255).all() and (src == 255).all()
    # no words
    dec, chars, src = S.decode_words_host(costs, [], [], np.zeros((66, 66), np.uint8))
    assert dec.shape == (0,) and chars.shape == (0, 64)


def test_argument_errors(S):
    B = np.zeros((66, 66), np.uint8)
    Cr = np.zeros((3, 65), np.uint8)
    for first, n_of in (([1], [3]), ([0], [-1]), ([-1], [1]), ([3], [1])):
        with pytest.raises(S.StrErError) as e:                           # a word outside the rows
            S.decode_words_host(Cr, first, n_of, B)
        assert e.value.code == -1
    for ins, dele in ((-1, 0), (0, 256), (256, 0), (0, -1)):
        with pytest.raises(S.StrErError) as e:
            S.decode_words_host(Cr, [0], [3], B, ins, dele)
        assert e.value.code == -1
    with pytest.raises(ValueError):
        S.decode_words_host(Cr, [0], [3], np.zeros((65, 65), np.uint8))
    L = S.load_library()
    one = np.zeros(1, np.int32)
    out, ch = np.zeros(1, S.WORD_DECODE_DTYPE), np.zeros(64, np.uint8)
    assert L.str_er_decode_words_host(Cr.ctypes.data, 3, one.ctypes.data, one.ctypes.data, 1, None, 0, 0, out.ctypes.data, ch.ctypes.data, ch.ctypes.data) == -1
    assert L.str_er_decode_words_host(Cr.ctypes.data, 3, one.ctypes.data, one.ctypes.data, 1, B.ctypes.data, 0, 0, None, ch.ctypes.data, ch.ctypes.data) == -1
    assert L.str_er_decode_words_host(None, 0, None, None, 0, B.ctypes.data, 0, 0, None, None, None) == 0
    assert L.str_er_set_bigram(None, B.ctypes.data) == -1 and L.str_er_set_word_decode(None, 0, 0) == -1 and L.str_er_bigram_info(None, None, None) == -1


def test_binding_constants_dtypes_and_keywords(S):
    assert S.WANT_WORD_DECODE == 1 << 23 == 8388608
    d = S.WORD_DECODE_DTYPE
    assert d.itemsize == 24 and tuple((n, d.fields[n][1]) for n in d.names) == RECORD
    for m in ("text_detect", "text_detect_list"):
        assert inspect.signature(getattr(S.ERFilter, m)).parameters["want_word_decode"].default is False
    for m in ("submit", "submit_nv12", "submit_copy", "submit_list", "submit_nv12_list", "submit_copy_list"):
        assert inspect.signature(getattr(S.FrameStream, m)).parameters["want_word_decode"].default is False
    binding = __import__("importlib").import_module("scene-text-recognition_amd.binding")
    assert binding._want_flags(word_decode=True) == 8388608 and binding._want_flags(run_read=True, word_match=True, word_decode=True) == 8388608 | 4194304 | 2097152
    assert binding._want_flags(word_match=True) == 4194304
    for m in ("set_bigram", "bigram_info", "set_word_decode", "decode_words"):
        assert callable(getattr(S.ERFilter, m)), m
    assert callable(S.FrameStream.set_bigram) and callable(S.FrameStream.set_word_decode)
    sig = inspect.signature(S.ERFilter.set_word_decode).parameters
    assert sig["ins"].default == 0 and sig["dele"].default == 0
    assert inspect.signature(S.bigram_from_words).parameters["alpha"].default == 1.0
    for m in ("bigram_from_probs", "bigram_from_words", "load_tp_table", "decode_words_host"):
        assert callable(getattr(S, m)), m
    for m in ("word_decodes", "word_decode_chars", "word_decode_src"):
        assert isinstance(getattr(S.Result, m), property)
    for m in ("word_decode_text", "word_decode_runs", "words_decode_text_of_line", "frame_line_decode_text"):
        assert callable(getattr(S.Result, m))


def test_result_accessors_without_the_flag(S):
    r = S.Result.__new__(S.Result)
    r._word_decodes = r._word_decode_chars = r._word_decode_src = r._run_costs = r._run_probs = None
    for name in ("word_decodes", "word_decode_chars", "word_decode_src", "run_costs", "run_probs"):
        with pytest.raises(ValueError):
            getattr(r, name)
    L = S.load_library()
    n = C.c_int32(7)
    assert L.str_er_result_word_decodes(None, n) is None and n.value == 0
    for fn in (L.str_er_result_word_decode_chars, L.str_er_result_word_decode_src):
        nb = C.c_uint64(7)
        assert fn(None, nb) is None and nb.value == 0


def test_text_accessors_on_a_made_up_result(S):
    """word_decode_text / word_decode_runs from the tables alone: a decoded word with an inserted character, and one that was not decoded."""
    r = S.Result.__new__(S.Result)
    r._words = np.zeros(2, S.LINE_WORD_DTYPE)
    r._words["first_run"], r._words["n_runs"] = [0, 2], [2, 1]
    r._run_reads = np.zeros(3, S.RUN_READ_DTYPE)
    r._run_reads["ch"] = [ord("A"), ord("B"), ord("Z")]
    r._word_decodes = np.zeros(2, S.WORD_DECODE_DTYPE)
    r._word_decodes["cost"], r._word_decodes["n_chars"] = [9, -1], [3, 0]
    r._word_decode_chars = np.full((2, 64), 255, np.uint8)
    r._word_decode_src = np.full((2, 64), 255, np.uint8)
    r._word_decode_chars[0, :3] = [WM.LABEL_OF["a"], WM.LABEL_OF["("], WM.LABEL_OF["7"]]
    r._word_decode_src[0, :3] = [0, 0x80, 1]
    assert r.word_decode_text(0) == "a(7" and r.word_decode_runs(0) == [(0, False), (0, True), (1, False)]
    assert r.word_decode_text(1) == "Z" and r.word_decode_runs(1) == [(2, False)]


def test_cpp_mirror_and_example_compile():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HOST, "example_word_decode.cpp")], check=True)
