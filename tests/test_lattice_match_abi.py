"""CPU checks of the lexicon match over the piece lattice (STR_ER_WANT_LATTICE_MATCH, str_er_lattice_match_words; the contract is at
str_er_lattice_match): header, record layout, exports, binding, the C++ mirror and example, and the pure host entry point
str_er_lattice_match_words_host against the reference (lattice_match_ref.py), every value with ==, with every validation and
capacity code."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import lattice_match_ref as LM
import word_match_ref as WM
from test_lattice_decode_abi import cheapen, make_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
HOST = os.path.join(ROOT, "scene-text-recognition_amd", "host")
FUNCS = ("str_er_lattice_match_words", "str_er_lattice_match_words_host", "str_er_lattice_match_stats", "str_er_result_lattice_matches",
         "str_er_result_lattice_match_src", "str_er_result_lattice_match_parts")
RECORD = (("entry", 0), ("cost", 4), ("second_entry", 8), ("second_cost", 12), ("free_cost", 16), ("n_tried", 20), ("first_part", 24), ("n_parts", 28),
          ("n_del", 32), ("n_ins", 36))
PARAMS = ((64, 64, 2, 8), (1, 1, 0, 0), (255, 255, 31, 255), (3, 200, 1, 8))          # INS, DEL, band, SPLIT


def test_header_declares_the_flag_the_record_and_the_prototypes():
    full = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert re.search(r"#define\s+STR_ER_WANT_LATTICE_MATCH\s+\(134217728u\)", txt)
    assert re.search(r"#define\s+STR_ER_ABI_VERSION\s+2\b", txt)
    assert re.search(r"typedef\s+struct\s+str_er_lattice_match\s*\{\s*int32_t\s+entry,\s*cost;\s*int32_t\s+second_entry,\s*second_cost;\s*int32_t\s+free_cost,\s*n_tried;"
                     r"\s*int32_t\s+first_part,\s*n_parts;\s*int32_t\s+n_del,\s*n_ins;\s*\}\s*str_er_lattice_match;", txt)
    for name in FUNCS:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
    flat = re.sub(r"\s*\n \*\s*", " ", full)
    for words in ("A definition of this library; integers only, exact", "Lattice: that of str_er_lattice_decode", "s = SPLIT if i > 0, else 0; no edge crosses a run boundary",
                  "a row is read as min(C[a], C[a'])", "D[0][0] = 0 and D[0][j] = j * INS", "in this order: for i = 0 .. jl - 1 ascending",
                  "SUB(i) = D[f][j - 1] + C_{r,i,jl}[e_j] + s, only for j >= 1; then DEL(i) = D[f][j] + DEL + s; last INS = D[n][j - 1] + INS, only for j >= 1",
                  "plus SPLIT * (|P| - n_runs)", "max(1, R - band) <= l <= min(32, N + band)", "A word with N > 32 tries nothing",
                  "behaves as the matcher does for m = 0", "it is made for every word, also for N > 32",
                  "the first candidate in the order above that attains D[n][j] is the move taken", "piece = -1 for a whole run",
                  "n_parts, n_del and n_ins are 0 where entry is -1", "n_parts - n_del + n_ins = l", "32 bytes per word, padded with 0xFF",
                  "0x80 | (the number of parts that end at or before the node it was inserted at)",
                  "the first six fields equal str_er_word_match's on the runs, field for field", "SPLIT * (n_parts of that sequence - n_runs)",
                  "pooling lattices over a word track is not part of this", "no bigram table enters",
                  # the two sentences that said the matcher had no such output point at it
                  "the lexicon over the same lattice is a separate output, str_er_lattice_match (STR_ER_WANT_LATTICE_MATCH)",
                  "against the lexicon, str_er_lattice_match (STR_ER_WANT_LATTICE_MATCH): every entry over all pieces of the word"):
        assert words in flat, words
    assert "no lexicon enters: the matcher still reads" not in flat


def test_record_layout_c99(tmp_path):
    src = tmp_path / "t.c"
    at = " && ".join(f"offsetof(str_er_lattice_match, {f}) == {o}" for f, o in RECORD)
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n'
                   f"typedef char rec_ok[sizeof(str_er_lattice_match) == 40 && {at} ? 1 : -1];\n"
                   "typedef char fl[STR_ER_WANT_LATTICE_MATCH == 134217728u && STR_ER_WANT_LATTICE_MATCH == (1u << 27) && STR_ER_WANT_LATTICE_DECODE == (1u << 26) ? 1 : -1];\n"
                   "int main(void) { rec_ok a; fl b;\n"
                   "  int (*g)(str_er_ctx *, const str_er_run_split *, int32_t, const uint8_t *, const uint8_t *, int32_t, const int32_t *, const int32_t *, int32_t,\n"
                   "           str_er_lattice_match *, uint8_t *, str_er_split_part *, int32_t, int32_t *) = str_er_lattice_match_words;\n"
                   "  int (*k)(const str_er_run_split *, int32_t, const uint8_t *, const uint8_t *, int32_t, const int32_t *, const int32_t *, int32_t, const char *,\n"
                   "           const int32_t *, int32_t, uint32_t, int32_t, int32_t, int32_t, int32_t, str_er_lattice_match *, uint8_t *, str_er_split_part *, int32_t,\n"
                   "           int32_t *) = str_er_lattice_match_words_host;\n"
                   "  int (*j)(const str_er_ctx *, uint64_t *) = str_er_lattice_match_stats;\n"
                   "  const str_er_lattice_match *(*p)(const str_er_result *, int32_t *) = str_er_result_lattice_matches;\n"
                   "  const uint8_t *(*q)(const str_er_result *, uint64_t *) = str_er_result_lattice_match_src;\n"
                   "  const str_er_split_part *(*r)(const str_er_result *, int32_t *) = str_er_result_lattice_match_parts;\n"
                   "  (void)a; (void)b; (void)g; (void)j; (void)k; (void)p; (void)q; (void)r; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_library_exports_the_symbols(S):
    L = S.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS:
        assert hasattr(L, name) and re.search(r"\bT\s+" + name + r"\b", out), name
    syms = subprocess.run(["nm", "-C", S.lib_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bk_lattice_match\b", syms) and re.search(r"\bk_lattice_match_final\b", syms)


def random_lexicon(rng, n, lo=1, hi=12):
    return ["".join(WM.ALPHABET[a] for a in rng.integers(0, 65, int(l))) for l in rng.integers(lo, hi + 1, n)]


def same(S, got, want):
    rec, src, parts = got
    assert rec.dtype == S.LATTICE_MATCH_DTYPE and parts.dtype == S.SPLIT_PART_DTYPE and src.shape == (len(rec), 32)
    assert LM.as_tuples(rec) == want[0]
    assert (src == want[1]).all()
    assert np.stack([parts["run"], parts["piece"]], 1).tolist() == want[2].tolist()


def test_host_equals_the_reference_on_random_words(S):
    rng = np.random.default_rng(41)
    n_of = np.array([0, 1, 2, 8, 13, 32, 33] + list(rng.integers(0, 7, 14)))
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]])
    cuts = rng.integers(0, 4, int(n_of.sum()))
    cuts[first[5]:first[5] + 32] = 0                                      # (32 uncut runs: N = 32 exactly; 33: nothing tried, free_cost still made)
    cuts[first[6]:first[6] + 33] = 0
    sp, rc, pc = make_rows(S, rng, cuts)
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    words = random_lexicon(rng, 150) + ["a" * 32, "B" * 31, "c" * 30]
    for fold in (True, False):
        lex = WM.Lexicon(words, fold)
        for ins, dele, band, split in PARAMS:
            want = LM.match_words(sp, rc, pc, first, n_of, lex, ins, dele, band, split)
            same(S, S.lattice_match_words_host(sp, rc, pc, first, n_of, words, fold, ins, dele, band, split), want)
            assert want[0][6][:4] == (-1, -1, -1, -1) and want[0][6][5] == 0 and want[0][6][7] == 0
            assert want[0][6][4] == int(rc[first[6]:first[6] + 33].min(axis=1).astype(np.int64).sum())
        assert want[0][5][0] >= 0                                         # (band 1 around 32 runs: the long entries)
    # no words, words without runs, and an empty lexicon
    rec, src, parts = S.lattice_match_words_host(sp, rc, pc, [], [], words)
    assert rec.shape == (0,) and src.shape == (0, 32) and parts.shape == (0,)
    rec, src, parts = S.lattice_match_words_host(sp[:0], rc[:0], pc[:0], [0, 0], [0, 0], ["ab", "c", "dE"], True, 7, 9, 2, 8)
    assert LM.as_tuples(rec) == [(1, 7, 0, 14, 0, 3, 0, 0, 0, 1)] * 2 and len(parts) == 0 and src[0, :2].tolist() == [0x80, 0xFF]
    rec, src, parts = S.lattice_match_words_host(sp, rc, pc, first[:5], n_of[:5], [])
    assert [r[:4] + r[5:] for r in LM.as_tuples(rec)] == [(-1, -1, -1, -1, 0, 0, 0, 0, 0)] * 5 and (src == 0xFF).all() and len(parts) == 0


def test_without_cuts_the_host_equals_the_word_matcher(S):
    rng = np.random.default_rng(42)
    n_of = np.array([0, 1, 5, 32, 33, 7])
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]])
    sp, rc, pc = make_rows(S, rng, np.zeros(int(n_of.sum()), np.int64))
    rc = cheapen(rng, rc)
    words = random_lexicon(rng, 200, 1, 9) + ["x" * 32, "Y" * 31]
    for fold in (True, False):
        for ins, dele, band, split in PARAMS:
            rec, src, parts = S.lattice_match_words_host(sp, rc, pc, first, n_of, words, fold, ins, dele, band, split)
            plain = S.match_words_host(rc, first, n_of, words, fold, ins, dele, band)
            assert [r[:6] for r in LM.as_tuples(rec)] == WM.as_tuples(plain)
            runs = [r for w in range(len(n_of)) if rec["entry"][w] >= 0 for r in range(first[w], first[w] + n_of[w])]
            assert parts["run"].tolist() == runs and (parts["piece"] == -1).all()


def test_argument_and_capacity_errors(S):
    rng = np.random.default_rng(43)
    words = ["ab", "cde", "f"]
    sp, rc, pc = make_rows(S, rng, [1, 0, 3])
    for first, n_of in (([1], [3]), ([0], [-1]), ([-1], [1]), ([3], [1])):
        with pytest.raises(S.StrErError) as e:                           # a word outside the runs
            S.lattice_match_words_host(sp, rc, pc, first, n_of, words)
        assert e.value.code == -1
    for field, value in (("n_cuts", 4), ("n_cuts", -1), ("n_pieces", 3), ("first_piece", -1), ("first_piece", len(pc) - 1)):
        bad = sp.copy()
        bad[field][0] = value                                            # cuts outside 0 .. 3, pieces that do not follow, pieces outside the rows
        with pytest.raises(S.StrErError) as e:
            S.lattice_match_words_host(bad, rc, pc, [0], [3], words)
        assert e.value.code == -1, (field, value)
    for ins, dele, band, split in ((0, 64, 2, 8), (64, 256, 2, 8), (256, 64, 2, 8), (64, 0, 2, 8), (64, 64, -1, 8), (64, 64, 32, 8), (64, 64, 2, -1), (64, 64, 2, 256)):
        with pytest.raises(S.StrErError) as e:                           # a bad INS, DEL, band or SPLIT
            S.lattice_match_words_host(sp, rc, pc, [0], [3], words, True, ins, dele, band, split)
        assert e.value.code == -1
    # the raw entry point: a lexicon byte outside the alphabet, NULL arguments, and cap_parts too small with *n_parts still set
    L = S.load_library()
    fr, no = np.zeros(1, np.int32), np.full(1, 3, np.int32)
    rec, sr, parts, n = np.zeros(1, S.LATTICE_MATCH_DTYPE), np.zeros(32, np.uint8), np.zeros(8, S.SPLIT_PART_DTYPE), C.c_int32(-5)
    raw, off = np.frombuffer(b"abcdef", np.uint8).copy(), np.array([0, 2, 5, 6], np.int32)
    p = lambda a: a.ctypes.data
    good = [p(sp), 3, p(rc), p(pc), len(pc), p(fr), p(no), 1, p(raw), p(off), 3, 1, 64, 64, 2, 8, p(rec), p(sr), p(parts), 8, C.byref(n)]
    assert L.str_er_lattice_match_words_host(*good) == 0 and 3 <= n.value <= 7 and int(rec["n_parts"][0]) == n.value and int(rec["entry"][0]) >= 0
    want = n.value
    for at in (0, 2, 3, 5, 6, 8, 9, 16, 17, 18, 20):
        bad = list(good)
        bad[at] = None
        assert L.str_er_lattice_match_words_host(*bad) == -1, at
    for at, value in ((1, -1), (4, -1), (7, -1), (10, -1), (11, 2), (19, -1)):
        bad = list(good)
        bad[at] = value
        assert L.str_er_lattice_match_words_host(*bad) == -1, at
    dirty = raw.copy()
    dirty[3] = ord("-")
    bad = list(good)
    bad[8] = p(dirty)
    assert L.str_er_lattice_match_words_host(*bad) == -1
    small = list(good)
    small[19] = want - 1
    n.value = -5
    before = rec.copy()
    assert L.str_er_lattice_match_words_host(*small) == -7 and n.value == want and rec.tobytes() == before.tobytes()          # STR_ER_ECAPACITY
    assert L.str_er_lattice_match_words_host(None, 0, None, None, 0, None, None, 0, p(raw), p(off), 3, 1, 64, 64, 2, 8, None, None, None, 0, C.byref(n)) == 0 and n.value == 0
    # a NULL context
    assert L.str_er_lattice_match_words(None, *good[:8], *good[16:]) == -1 and L.str_er_lattice_match_stats(None, None) == -1


def test_binding_constants_dtypes_and_keywords(S):
    assert S.WANT_LATTICE_MATCH == 1 << 27 == 134217728
    d = S.LATTICE_MATCH_DTYPE
    assert d.itemsize == 40 and tuple((n, d.fields[n][1]) for n in d.names) == RECORD
    for m in ("text_detect", "text_detect_list"):
        assert inspect.signature(getattr(S.ERFilter, m)).parameters["want_lattice_match"].default is False
    for m in ("submit", "submit_nv12", "submit_copy", "submit_list", "submit_nv12_list", "submit_copy_list"):
        assert inspect.signature(getattr(S.FrameStream, m)).parameters["want_lattice_match"].default is False
    binding = __import__("importlib").import_module("scene-text-recognition_amd.binding")
    assert binding._want_flags(lattice_match=True) == 134217728
    assert binding._want_flags(run_split=True, word_match=True, lattice_match=True) == 134217728 | 16777216 | S.WANT_WORD_MATCH
    assert binding._want_flags(lattice_decode=True) == 67108864
    for m in ("lattice_match_words", "lattice_match_stats"):
        assert callable(getattr(S.ERFilter, m)), m
    assert callable(S.lattice_match_words_host)
    sig = inspect.signature(S.lattice_match_words_host).parameters
    assert (sig["fold_case"].default, sig["ins"].default, sig["dele"].default, sig["band"].default, sig["split_cost"].default) == (True, 64, 64, 2, 8)
    for m in ("lattice_matches", "lattice_match_src", "lattice_match_parts"):
        assert isinstance(getattr(S.Result, m), property)
    for m in ("word_lattice_match_text", "word_lattice_match_parts", "words_lattice_match_text_of_line", "frame_line_lattice_match_text"):
        assert callable(getattr(S.Result, m))


def test_result_accessors_without_the_flag(S):
    r = S.Result.__new__(S.Result)                                        # (a result made by hand with none of the new attributes)
    for name in ("lattice_matches", "lattice_match_src", "lattice_match_parts"):
        with pytest.raises(ValueError):
            getattr(r, name)
    L = S.load_library()
    for fn in (L.str_er_result_lattice_matches, L.str_er_result_lattice_match_parts):
        n = C.c_int32(7)
        assert fn(None, n) is None and n.value == 0
    nb = C.c_uint64(7)
    assert L.str_er_result_lattice_match_src(None, nb) is None and nb.value == 0


def test_text_accessors_on_a_made_up_result(S):
    """word_lattice_match_text / word_lattice_match_parts from the tables alone: a matched word and one without a match."""
    r = S.Result.__new__(S.Result)
    r._words = np.zeros(2, S.LINE_WORD_DTYPE)
    r._words["first_run"], r._words["n_runs"] = [0, 2], [2, 1]
    r._run_reads = np.zeros(3, S.RUN_READ_DTYPE)
    r._run_reads["ch"] = [ord("A"), ord("B"), ord("Z")]
    r._lexicon = ("corn", "com")
    r._lattice_matches = np.zeros(2, S.LATTICE_MATCH_DTYPE)
    r._lattice_matches["entry"], r._lattice_matches["cost"] = [0, -1], [9, -1]
    r._lattice_matches["first_part"], r._lattice_matches["n_parts"] = [0, 3], [3, 0]
    r._lattice_match_src = np.full((2, 32), 255, np.uint8)
    r._lattice_match_src[0, :4] = [0, 0x81, 1, 2]
    r._lattice_match_parts = np.array([(0, -1), (1, 0), (1, 1)], S.SPLIT_PART_DTYPE)
    assert r.word_lattice_match_text(0) == "corn" and r.word_lattice_match_parts(0).tolist() == [(0, -1), (1, 0), (1, 1)]
    assert r.word_lattice_match_text(1) == "Z" and len(r.word_lattice_match_parts(1)) == 0
    r._line_words = np.zeros(1, S.LINE_WORDS_DTYPE)
    r._line_words["first_word"], r._line_words["n_words"] = [0], [2]
    assert r.words_lattice_match_text_of_line(0) == ["corn", "Z"]


def test_cpp_mirror_and_example_compile():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HOST, "example_lattice_match.cpp")], check=True)
    txt = open(os.path.join(HOST, "er_filter_hip.hpp")).read()
    for name in ("lattice_match_words", "lattice_match_words_host", "word_lattice_match_text", "line_lattice_match_text", "lattice_matches") + FUNCS[:2] + FUNCS[3:]:
        assert re.search(r"\b" + name + r"\(", txt), name
