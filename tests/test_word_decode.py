"""The word decoder on the GPU (str_er_set_bigram, str_er_set_word_decode, str_er_decode_words; the contract is at
str_er_word_decode): every field of every record and every byte of the strings against the numpy reference (word_decode_ref.py) with
==, at the kernel's own edges -- the run counts around the matcher's buckets and the limit of 32, the words of a workgroup (a wave
each), the states 64 and 65 that live past the wave's 64 lanes, the tie rules on constant inputs.  The launch takes a workgroup per
group of words with no cap on the grid: there is no pass to overrun."""
import numpy as np
import pytest

import word_decode_ref as WD
import word_match_ref as WM
from test_word_decode_ref import PAIRS, insertion_vector

pytestmark = pytest.mark.gpu
WG_WORDS = 4                      # words of a workgroup of k_word_decode (WD_WORDS)


@pytest.fixture(scope="module")
def f(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    yield ctx
    ctx.close()


def _rows(rng, n):
    """Random cost rows: a few cheap characters per run among dear ones."""
    c = rng.integers(60, 256, (n, 65))
    cheap = rng.random((n, 65)) < 0.08
    c[cheap] = rng.integers(0, 24, int(cheap.sum()))
    return c.astype(np.uint8)


def _spans(n_of):
    n_of = np.asarray(n_of, np.int64)
    return np.concatenate([[0], np.cumsum(n_of)])[:len(n_of)].astype(np.int32), n_of.astype(np.int32)


def check(f, costs, first, n_of, B, ins=0, dele=0):
    """set_bigram, set_word_decode and decode_words against the reference; returns the records as tuples (DECODE_FIELDS), chars, src."""
    f.set_bigram(B)
    f.set_word_decode(ins, dele)
    dec, chars, src = f.decode_words(costs, first, n_of)
    want, wc, ws = WD.decode_words(costs, first, n_of, B, ins, dele)
    got = WD.as_tuples(dec)
    assert got == want, [(w, g, x) for w, (g, x) in enumerate(zip(got, want)) if g != x][:5]
    assert (chars == wc).all() and (src == ws).all(), np.argwhere((chars != wc) | (src != ws))[:5]
    return got, chars, src


@pytest.mark.parametrize("ins,dele", PAIRS)
def test_run_counts_under_every_pair_of_moves(f, ins, dele):
    rng = np.random.default_rng(1000 + ins + 7 * dele)
    first, n_of = _spans([0, 1, 2, 8, 9, 16, 17, 31, 32, 33])
    costs = _rows(rng, int(n_of.sum()))
    B = rng.integers(0, 256, (66, 66)).astype(np.uint8)
    got, chars, src = check(f, costs, first, n_of, B, ins, dele)
    assert got[0] == (int(B[65, 65]), int(B[65, 65]), 0, 0, 0, 0)
    assert got[9][0] == -1 and got[9][2:] == (0, 0, 0, 0) and got[9][1] > 0 and (chars[9] == 255).all()
    for g, m in zip(got[:9], n_of[:9]):
        assert g[0] <= g[1] and g[3] + g[5] == g[2] and g[3] + g[4] == m
    # a cheap table beside the dear rows, so that the moves are taken where they are on
    B2 = rng.integers(0, 6, (66, 66)).astype(np.uint8)
    got, _, _ = check(f, costs, first, n_of, B2, ins, dele)
    if 0 < ins < 255:
        assert sum(g[5] for g in got) > 0
    if 0 < dele < 255:
        assert sum(g[4] for g in got) > 0


def test_word_counts_around_a_workgroup(S, f):
    rng = np.random.default_rng(2)
    B = rng.integers(0, 64, (66, 66)).astype(np.uint8)
    for n in (0, 1, WG_WORDS - 1, WG_WORDS, WG_WORDS + 1, 257):
        first, n_of = _spans(rng.integers(0, 12, n))
        costs = _rows(rng, max(1, int(n_of.sum())))
        got, chars, src = check(f, costs, first, n_of, B, 20, 30)
        assert len(got) == n and chars.shape == (n, 64) and src.shape == (n, 64)
    dec, chars, src = f.decode_words(np.zeros((0, 65), np.uint8), [], [])
    assert dec.shape == (0,) and dec.dtype == S.WORD_DECODE_DTYPE


def test_constant_inputs_where_every_tie_rule_decides(f):
    for m in (1, 5, 32):
        first, n_of = _spans([m])
        zero, full = np.zeros((m, 65), np.uint8), np.full((m, 65), 255, np.uint8)
        for ins, dele in PAIRS:
            got, chars, src = check(f, zero, first, n_of, np.zeros((66, 66), np.uint8), ins, dele)
            assert got[0] == (0, 0, m, m, 0, 0) and (chars[0, :m] == 0).all() and src[0, :m].tolist() == list(range(m))
            check(f, full, first, n_of, np.full((66, 66), 255, np.uint8), ins, dele)
            check(f, zero, first, n_of, np.full((66, 66), 255, np.uint8), ins, dele)
            check(f, full, first, n_of, np.zeros((66, 66), np.uint8), ins, dele)
    # the vectors of the contract
    got, chars, src = check(f, np.zeros((5, 65), np.uint8), [0], [5], np.zeros((66, 66), np.uint8), 64, 64)
    assert got[0] == (0, 0, 5, 5, 0, 0) and src[0, :6].tolist() == [0, 1, 2, 3, 4, 255]
    full = np.full((33, 65), 255, np.uint8)
    got, chars, src = check(f, full, [0, 0], [32, 33], np.full((66, 66), 255, np.uint8), 255, 255)
    assert got == [(33 * 255, 65 * 255, 0, 0, 32, 0), (-1, 67 * 255, 0, 0, 0, 0)] and (chars == 255).all() and (src == 255).all()


def test_the_64_character_vector(f):
    C, B = insertion_vector()
    got, chars, src = check(f, C, [0], [32], B, 1, 0)
    assert got[0][0] == 32 and got[0][2:] == (64, 32, 0, 32)
    assert chars[0].tolist() == [63, 64] * 32 and src[0].tolist() == [v for i in range(32) for v in (i, 0x80 | i)]


def test_paths_through_the_states_past_the_wave(f):
    """Best paths that run through the labels 63 and 64 and lean on the boundary row and column."""
    rng = np.random.default_rng(3)
    # ")(" repeated: the rows say nothing (all equal), the table alone decides, from the boundary row to the boundary column
    m = 6
    rows = np.full((m, 65), 9, np.uint8)
    B = np.full((66, 66), 200, np.uint8)
    B[65, 64] = B[64, 63] = B[63, 64] = 1
    B[63, 65] = 2
    got, chars, src = check(f, rows, [0], [m], B)
    assert chars[0, :m].tolist() == [64, 63] * 3 and got[0][0] == m * 9 + 1 + 5 + 2
    # the same with a row that reads ')' dear: DEL takes it out, INS puts a ')' in behind a '('
    rows2 = rows.copy()
    rows2[2, :] = 250
    got, chars, src = check(f, rows2, [0], [m], B, 3, 4)
    assert got[0][4] >= 1
    # label 64 against label 0, a tie that the smallest state wins, and label 64 alone cheaper
    tie = np.full((3, 65), 100, np.uint8)
    tie[:, 0] = tie[:, 64] = 7
    got, chars, src = check(f, tie, [0], [3], np.zeros((66, 66), np.uint8))
    assert chars[0, :3].tolist() == [0, 0, 0]
    tie[:, 64] = 6
    got, chars, src = check(f, tie, [0], [3], np.zeros((66, 66), np.uint8))
    assert chars[0, :3].tolist() == [64, 64, 64]
    # ending on ')' is free and on anything else dear; beginning with '(' likewise: the boundary terms move the string
    B = np.zeros((66, 66), np.uint8)
    B[:65, 65] = 90
    B[64, 65] = 0
    B[65, :65] = 90
    B[65, 63] = 0
    flat = np.full((4, 65), 30, np.uint8)
    flat[:, 5] = 10
    got, chars, src = check(f, flat, [0], [4], B)
    assert chars[0, :4].tolist() == [63, 5, 5, 64] and got[0][0] == 30 + 10 + 10 + 30
    # INS of label 64 behind label 63, and of label 63 behind 64, on random rows with those two cheap
    rows = _rows(rng, 20)
    rows[:, 63] = rng.integers(0, 4, 20)
    rows[:, 64] = rng.integers(0, 4, 20)
    B = rng.integers(100, 256, (66, 66)).astype(np.uint8)
    B[63, 64] = B[64, 63] = B[65, 63] = B[65, 64] = B[63, 65] = B[64, 65] = 0
    first, n_of = _spans([20, 7, 1, 12])
    first[1:] = [0, 19, 4]
    got, chars, src = check(f, rows, first, n_of, B, 2, 2)
    assert set(chars[0, :got[0][2]].tolist()) <= {63, 64}


def test_plain_viterbi_on_a_zero_table_is_the_arg_min_string(S, f):
    rng = np.random.default_rng(4)
    first, n_of = _spans([5, 1, 32, 0, 17])
    costs = _rows(rng, int(n_of.sum()))
    got, chars, src = check(f, costs, first, n_of, np.zeros((66, 66), np.uint8))
    f.set_lexicon(["A"])
    free = [int(r["free_cost"]) for r in f.match_words(costs, first, n_of)]
    for w, (a, m) in enumerate(zip(first, n_of)):
        assert chars[w, :m].tolist() == costs[a:a + m].argmin(axis=1).tolist() and src[w, :m].tolist() == list(range(m))
        assert got[w][0] == got[w][1] == free[w] == int(costs[a:a + m].min(axis=1).astype(np.int64).sum())


def test_random_words_equal_the_host_rules_and_a_repeat_call(S, f):
    rng = np.random.default_rng(5)
    n_of = rng.integers(0, 33, 120)
    first, n_of = _spans(n_of)
    costs = _rows(rng, int(n_of.sum()))
    B = S.bigram_from_words(["".join(rng.choice(list(WM.ALPHABET), int(rng.integers(1, 9)))) for _ in range(300)])
    got, chars, src = check(f, costs, first, n_of, B, 64, 64)
    dec, c2, s2 = f.decode_words(costs, first, n_of)
    assert WD.as_tuples(dec) == got and c2.tobytes() == chars.tobytes() and s2.tobytes() == src.tobytes()
    hd, hc, hs = S.decode_words_host(costs, first, n_of, B, 64, 64)
    assert WD.as_tuples(hd) == got and (hc == chars).all() and (hs == src).all()
    # overlapping words are words too
    dec, c3, _ = f.decode_words(costs, [0, 0, 3], [5, 5, 6])
    assert dec[0].tobytes() == dec[1].tobytes() and c3[0].tobytes() == c3[1].tobytes()


def test_errors_leave_the_context_usable(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    try:
        costs = np.zeros((2, 65), np.uint8)
        assert ctx.bigram_info() == {"set": False, "device_bytes": 0}
        with pytest.raises(S.StrErError) as e:                           # no table
            ctx.decode_words(costs, [0], [2])
        assert e.value.code == -6 and "bigram" in str(e.value)
        B = np.zeros((66, 66), np.uint8)
        B[65, 65] = 3
        ctx.set_bigram(B)
        assert ctx.bigram_info()["set"] and ctx.bigram_info()["device_bytes"] >= 4356
        dec, chars, src = ctx.decode_words(costs, [0, 0], [2, 0])
        assert WD.as_tuples(dec) == [(0, 0, 2, 2, 0, 0), (3, 3, 0, 0, 0, 0)]
        for ins, dele in ((-1, 0), (0, 256), (256, 0)):
            with pytest.raises(S.StrErError) as e:
                ctx.set_word_decode(ins, dele)
            assert e.value.code == -1
        for first, n_of in (([1], [2]), ([0], [-1]), ([-1], [1])):
            with pytest.raises(S.StrErError) as e:                       # a word outside the cost rows
                ctx.decode_words(costs, first, n_of)
            assert e.value.code == -1
        again = ctx.decode_words(costs, [0, 0], [2, 0])
        assert again[0].tobytes() == dec.tobytes() and again[1].tobytes() == chars.tobytes()
        ctx.set_bigram(None)                                             # removed
        assert ctx.bigram_info() == {"set": False, "device_bytes": 0}
        with pytest.raises(S.StrErError) as e:
            ctx.decode_words(costs, [0], [2])
        assert e.value.code == -6
    finally:
        ctx.close()
