"""CPU checks of the lexicon matcher (STR_ER_WANT_WORD_MATCH, str_er_set_lexicon, str_er_match_words; the contract is at
str_er_word_match): header, record layout, exports, binding, the C++ mirror and example, and the pure host entry points --
str_er_cost_thresholds, str_er_prob_costs, str_er_match_words_host -- against the reference (word_match_ref.py), every value with ==."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import word_match_ref as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
HOST = os.path.join(ROOT, "scene-text-recognition_amd", "host")
FUNCS = ("str_er_set_lexicon", "str_er_lexicon_info", "str_er_set_word_match", "str_er_cost_thresholds", "str_er_prob_costs", "str_er_run_costs",
         "str_er_match_words", "str_er_match_words_host", "str_er_result_word_matches", "str_er_result_run_costs", "str_er_result_run_probs")
MATCH = (("entry", 0), ("cost", 4), ("second_entry", 8), ("second_cost", 12), ("free_cost", 16), ("n_tried", 20))


def test_header_declares_the_flag_the_record_and_the_prototypes():
    full = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert re.search(r"#define\s+STR_ER_WANT_WORD_MATCH\s+\(4194304u\)", txt)
    assert re.search(r"#define\s+STR_ER_LEXICON_FOLD_CASE\s+1u", txt)
    assert re.search(r"typedef\s+struct\s+str_er_word_match\s*\{\s*int32_t\s+entry,\s*cost;\s*int32_t\s+second_entry,\s*second_cost;\s*int32_t\s+free_cost,\s*n_tried;"
                     r"\s*\}\s*str_er_word_match;", txt)
    for name in FUNCS:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
    flat = re.sub(r"\s*\n \*\s*", " ", full)
    for words in ("smallest c in 0 .. 254 with p >= T[c]", "The unit is 1/8 bit", "D[i][j] = min(D[i-1][j-1] + C_i[e_j], D[i-1][j] + DEL, D[i][j-1] + INS)",
                  "|l - m| <= band", "A word with m > 32 tries nothing", "touching glyphs reads as one character"):
        assert words in flat, words


def test_record_layout_c99(tmp_path):
    src = tmp_path / "t.c"
    at = " && ".join(f"offsetof(str_er_word_match, {f}) == {o}" for f, o in MATCH)
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n'
                   f"typedef char match_ok[sizeof(str_er_word_match) == 24 && {at} ? 1 : -1];\n"
                   "typedef char fl[STR_ER_WANT_WORD_MATCH == 4194304u && STR_ER_WANT_WORD_MATCH == (1u << 22) && STR_ER_WANT_RUN_READ == (1u << 21) ? 1 : -1];\n"
                   "int main(void) { match_ok a; fl b;\n"
                   "  int (*f)(str_er_ctx *, const char *, const int32_t *, int32_t, uint32_t) = str_er_set_lexicon;\n"
                   "  int (*g)(str_er_ctx *, const uint8_t *, int32_t, const int32_t *, const int32_t *, int32_t, str_er_word_match *) = str_er_match_words;\n"
                   "  int (*h)(const double *, int32_t, int32_t, const int32_t *, int32_t, uint8_t *) = str_er_prob_costs;\n"
                   "  const str_er_word_match *(*p)(const str_er_result *, int32_t *) = str_er_result_word_matches;\n"
                   "  const double *(*q)(const str_er_result *, uint64_t *) = str_er_result_run_probs;\n"
                   "  (void)a; (void)b; (void)f; (void)g; (void)h; (void)p; (void)q; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_library_exports_the_symbols(S):
    L = S.load_library()
    for name in FUNCS:
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS:
        assert re.search(r"\bT\s+" + name + r"\b", out), name
    syms = subprocess.run(["nm", "-C", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for kernel in ("k_run_costs", "k_word_match", "k_word_match_final"):
        assert re.search(r"\b" + kernel + r"\b", syms), kernel


def test_cost_thresholds_equal_the_reference_table(S):
    got = S.cost_thresholds()
    assert got.dtype == np.float64 and got.shape == (255,)
    assert got.tobytes() == WM.T.tobytes()


def _boundary_probs():
    """Every threshold, one step below and above it, and the values the contract names."""
    below, above = np.nextafter(WM.T, 0.0), np.nextafter(WM.T, 2.0)
    extra = np.array([0.0, -0.0, 1.0, 2.0, np.nan, -1.0, np.inf, -np.inf, 5e-324, 0.5, 0.3, 1e-12])
    return np.concatenate([WM.T, below, above, extra])


def test_prob_costs_on_the_boundary_values(S):
    p = _boundary_probs()
    want = np.concatenate([np.arange(255), np.minimum(np.arange(255) + 1, 255), np.arange(255)])
    assert (WM.cost(p)[:765] == want).all()                           # the reference itself, against the definition
    assert (WM.cost(p)[765:771] == [255, 255, 0, 0, 255, 255]).all()
    # one class per run that carries the value: label a = i % 65
    k = 65
    prob = np.zeros((len(p), k))
    prob[np.arange(len(p)), np.arange(len(p)) % k] = p
    labels = np.arange(k)
    got = S.prob_costs(prob, labels)
    assert got.shape == (len(p), 65) and got.dtype == np.uint8
    assert (got == WM.cost_rows(prob, labels)).all()
    assert (got[np.arange(len(p)), np.arange(len(p)) % k] == WM.cost(p)).all()


def test_prob_costs_labels_and_fold(S):
    rng = np.random.default_rng(5)
    n = 40
    cases = {
        "permuted": rng.permutation(65),
        "outside": np.array([3, 70, -1, 64, 65, 2 ** 31 - 1, 10, 36, -2 ** 31]),
        "missing": np.array([a for a in range(65) if a not in (11, 37, 62)]),          # no 'B', no 'b', no '&'
        "twice": np.array([10, 36, 10, 5]),
        "none": np.zeros(0, np.int64),
    }
    for name, labels in cases.items():
        prob = np.exp2(-rng.uniform(0, 34, (n, len(labels))))
        prob[rng.random(prob.shape) < 0.1] = 0.0
        if prob.size:
            prob[0, 0] = np.nan
        for fold in (False, True):
            want = WM.cost_rows(prob, labels, fold)
            got = S.prob_costs(prob, labels, fold)
            assert (got == want).all(), (name, fold)
    # what the cases are about
    labels = cases["missing"]
    prob = np.full((1, len(labels)), 0.5)
    prob[0, list(labels).index(10)] = 0.25                            # 'A' at 16, 'a' at 8
    got = S.prob_costs(prob, labels)[0]
    assert got[11] == got[37] == got[62] == 255 and got[10] == 16 and got[36] == 8
    got = S.prob_costs(prob, labels, fold=True)[0]
    assert got[10] == got[36] == 8 and got[11] == got[37] == 255
    got = S.prob_costs(np.array([[1.0, 0.5, 0.25, 0.125]]), cases["twice"])[0]
    assert got[10] == 0 and got[36] == 8 and got[5] == 24             # the first class with a label counts
    L = S.load_library()
    assert L.str_er_prob_costs(None, 1, 1, None, 0, None) == -1 and L.str_er_prob_costs(None, -1, 0, None, 0, None) == -1
    assert L.str_er_prob_costs(None, 0, 0, None, 0, None) == 0


def test_match_words_host_equals_the_reference(S):
    rng = np.random.default_rng(11)
    words = ["".join(rng.choice(list(WM.ALPHABET), int(rng.integers(1, 9)))) for _ in range(300)] + ["HOTEL", "hotel", "HOTEL"]
    n_of = rng.integers(0, 9, 30)
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]])
    costs = np.where(rng.random((int(n_of.sum()), 65)) < 0.1, rng.integers(0, 16, (int(n_of.sum()), 65)), rng.integers(0, 256, (int(n_of.sum()), 65))).astype(np.uint8)
    for fold, ins, dele, band in ((True, 64, 64, 2), (False, 64, 64, 2), (True, 1, 255, 0), (False, 200, 3, 31)):
        want = WM.match_words(costs, first, n_of, WM.Lexicon(words, fold), ins, dele, band)
        got = S.match_words_host(costs, first, n_of, words, fold, ins, dele, band)
        assert WM.as_tuples(got) == want, (fold, ins, dele, band)
    # HOTEL with a 0 for the O: the lexicon reads it, the arg max does not
    C = np.full((5, 65), 255, np.uint8)
    for i, ch in enumerate("H0TEL"):
        C[i, WM.LABEL_OF[ch]] = 2
    C[1, WM.LABEL_OF["O"]] = 9
    got = S.match_words_host(C, [0], [5], words, True)[0]
    assert (int(got["entry"]), int(got["cost"]), int(got["second_entry"]), int(got["second_cost"]), int(got["free_cost"])) == (300, 17, 301, 17, 10)
    for bad in (["A B"], [""], ["A" * 33]):
        with pytest.raises(S.StrErError) as e:
            S.match_words_host(C, [0], [5], bad)
        assert e.value.code == -1
    with pytest.raises(S.StrErError):
        S.match_words_host(C, [3], [3], words)                        # a word outside the rows


def test_binding_constants_dtypes_and_keywords(S):
    assert S.WANT_WORD_MATCH == 1 << 22 == 4194304 and S.LEXICON_FOLD_CASE == 1
    d = S.WORD_MATCH_DTYPE
    assert d.itemsize == 24 and tuple((n, d.fields[n][1]) for n in d.names) == MATCH
    for m in ("text_detect", "text_detect_list"):
        assert inspect.signature(getattr(S.ERFilter, m)).parameters["want_word_match"].default is False
    for m in ("submit", "submit_nv12", "submit_copy", "submit_list", "submit_nv12_list", "submit_copy_list"):
        assert inspect.signature(getattr(S.FrameStream, m)).parameters["want_word_match"].default is False
    binding = __import__("importlib").import_module("scene-text-recognition_amd.binding")
    assert binding._want_flags(word_match=True) == 4194304 and binding._want_flags(run_read=True, word_match=True) == 4194304 | 2097152
    for m in ("set_lexicon", "set_word_match", "match_words", "run_costs", "lexicon_info"):
        assert callable(getattr(S.ERFilter, m)), m
    assert callable(S.FrameStream.set_lexicon) and callable(S.FrameStream.set_word_match)
    assert inspect.signature(S.ERFilter.set_lexicon).parameters["fold_case"].default is True
    for m in ("word_matches", "run_costs", "run_probs"):
        assert isinstance(getattr(S.Result, m), property)
    for m in ("word_match_text", "words_match_text_of_line", "frame_line_match_text"):
        assert callable(getattr(S.Result, m))


def test_result_accessors_without_the_flag(S):
    r = S.Result.__new__(S.Result)
    r._word_matches = r._run_costs = r._run_probs = None
    for name in ("word_matches", "run_costs", "run_probs"):
        with pytest.raises(ValueError):
            getattr(r, name)
    L = S.load_library()
    n = C.c_int32(7)
    assert L.str_er_result_word_matches(None, n) is None and n.value == 0
    for fn in (L.str_er_result_run_costs, L.str_er_result_run_probs):
        nb = C.c_uint64(7)
        assert fn(None, nb) is None and nb.value == 0


def test_cpp_mirror_and_example_compile():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HOST, "example_word_match.cpp")], check=True)
