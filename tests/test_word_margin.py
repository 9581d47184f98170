"""The word decoder's margins on the GPU (str_er_word_margins; the contract is at str_er_word_margin): every field of every record,
every row margin, reading and alternative and the full table of marginals against the numpy reference (word_margin_ref.py) with ==, at
the kernel's own edges -- the run counts up to and past the limit of 32, the words of a workgroup (a wave each), the states 64 and 65
that live past the wave's 64 lanes, the drop entry, the largest values the 16-bit copies of the forward pass must hold."""
import os
import re

import numpy as np
import pytest

import word_margin_ref as WG
from test_word_decode_ref import PAIRS, insertion_vector

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WG_WORDS = 4                      # words of a workgroup of k_word_margin (WG_WORDS)


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
    """set_bigram, set_word_decode and word_margins against the reference, with and without the marginals; returns the records as
    tuples (MARGIN_FIELDS), row_margin, row_read, row_alt, marginals."""
    f.set_bigram(B)
    f.set_word_decode(ins, dele)
    rec, rm, rr, ra, mg = f.word_margins(costs, first, n_of, want_marginals=True)
    want, wm, wr, wa, wg = WG.word_margins(costs, first, n_of, B, ins, dele)
    got = WG.as_tuples(rec)
    assert got == want, [(w, g, x) for w, (g, x) in enumerate(zip(got, want)) if g != x][:5]
    assert (rm == wm).all() and (rr == wr).all() and (ra == wa).all(), (np.argwhere(rm != wm)[:5], np.argwhere(rr != wr)[:5], np.argwhere(ra != wa)[:5])
    assert (mg == wg).all(), np.argwhere(mg != wg)[:5]
    rec2, rm2, rr2, ra2, none = f.word_margins(costs, first, n_of)
    assert none is None and rec2.tobytes() == rec.tobytes() and rm2.tobytes() == rm.tobytes() and rr2.tobytes() == rr.tobytes() and ra2.tobytes() == ra.tobytes()
    return got, rm, rr, ra, mg


def test_the_words_of_a_workgroup_are_the_header_s():
    with open(os.path.join(ROOT, "scene-text-recognition_amd", "csrc", "word_margin_kernels.h")) as h:
        assert int(re.search(r"constexpr int WG_WORDS = (\d+);", h.read()).group(1)) == WG_WORDS


@pytest.mark.parametrize("ins,dele", PAIRS)
def test_run_counts_under_every_pair_of_moves(f, ins, dele):
    rng = np.random.default_rng(1100 + ins + 7 * dele)
    first, n_of = _spans([0, 1, 2, 8, 9, 16, 17, 31, 32, 33])
    costs = _rows(rng, int(n_of.sum()))
    B = rng.integers(0, 256, (66, 66)).astype(np.uint8)
    got, rm, rr, ra, mg = check(f, costs, first, n_of, B, ins, dele)
    for w in (0, 9):                                             # no rows, and not decoded
        assert got[w] == (-1, -1, -1, -1) and (rm[w] == -1).all() and (rr[w] == 255).all() and (ra[w] == 255).all() and (mg[w] == -1).all()
    for w, m in list(enumerate(n_of))[1:9]:
        assert got[w][0] == rm[w, :m].min() >= 0 and (rm[w, m:] == -1).all() and (rr[w, :m] <= 65).all() and (rr[w, m:] == 255).all()
        assert ((mg[w, :m, 65] >= 0) == (dele > 0)).all() and (mg[w, :m, :65] >= 0).all() and (mg[w, m:] == -1).all()
    # a cheap table beside the dear rows, so that the moves are taken where they are on: the drop entry is read and is the alternative
    B2 = rng.integers(0, 6, (66, 66)).astype(np.uint8)
    got, rm, rr, ra, mg = check(f, costs, first, n_of, B2, ins, dele)
    if 0 < dele < 255:
        assert (rr == 65).any() and (ra == 65).any()


def test_word_counts_around_a_workgroup(S, f):
    rng = np.random.default_rng(12)
    B = rng.integers(0, 64, (66, 66)).astype(np.uint8)
    for n in (0, 1, WG_WORDS - 1, WG_WORDS, WG_WORDS + 1, 257):
        first, n_of = _spans(rng.integers(0, 12, n))
        costs = _rows(rng, max(1, int(n_of.sum())))
        got, rm, rr, ra, mg = check(f, costs, first, n_of, B, 20, 30)
        assert len(got) == n and rm.shape == (n, 32) and rr.shape == (n, 32) and ra.shape == (n, 32) and mg.shape == (n, 32, 66)
    rec, rm, rr, ra, mg = f.word_margins(np.zeros((0, 65), np.uint8), [], [], want_marginals=True)
    assert rec.shape == (0,) and rec.dtype == S.WORD_MARGIN_DTYPE and mg.shape == (0, 32, 66)


def test_constant_inputs(f):
    zero_t, full_t = np.zeros((66, 66), np.uint8), np.full((66, 66), 255, np.uint8)
    for m in (1, 5, 32):
        first, n_of = _spans([m])
        for ins, dele in PAIRS:                                   # all zero: every margin is 0, the reading 0, the alternative 1
            got, rm, rr, ra, mg = check(f, np.zeros((m, 65), np.uint8), first, n_of, zero_t, ins, dele)
            assert got[0] == (0, 0, 0, 1) and (rm[0, :m] == 0).all() and (rr[0, :m] == 0).all() and (ra[0, :m] == 1).all()
    # all 255 at 32 rows: the largest values there are -- a narrow copy in LDS or a sentinel that collides shows here
    first, n_of = _spans([32])
    full = np.full((32, 65), 255, np.uint8)
    got, rm, rr, ra, mg = check(f, full, first, n_of, full_t, 0, 0)
    assert (mg[0, :, :65] == 16575).all() and (mg[0, :, 65] == -1).all() and got[0] == (0, 0, 0, 1)
    got, rm, rr, ra, mg = check(f, full, first, n_of, full_t, 255, 255)
    assert got[0] == (255, 0, 65, 0) and (mg[0, :, 65] == 33 * 255).all() and (rr[0] == 65).all() and int(mg.max()) <= 16575
    check(f, full, first, n_of, zero_t, 255, 255)
    check(f, np.zeros((32, 65), np.uint8), first, n_of, full_t, 255, 255)


def test_paths_through_the_states_past_the_wave(f):
    """The ")(" vector of the decoder's tests and its DEL / INS variant: readings and alternatives among 63, 64 and 65."""
    m = 6
    rows = np.full((m, 65), 9, np.uint8)
    B = np.full((66, 66), 200, np.uint8)
    B[65, 64] = B[64, 63] = B[63, 64] = 1
    B[63, 65] = 2
    got, rm, rr, ra, mg = check(f, rows, [0], [m], B)
    assert rr[0, :m].tolist() == [64, 63] * 3 and (rm[0, :m] > 0).all()
    rows2 = rows.copy()
    rows2[2, :] = 250
    got, rm, rr, ra, mg = check(f, rows2, [0], [m], B, 3, 4)
    assert set(rr[0, :m].tolist()) <= {63, 64, 65} and 65 in rr[0, :m].tolist()
    assert set(ra[0, :m].tolist()) & {63, 64, 65}
    # label 64 against label 0 on a zero table: a tie, the reading 0 and the alternative 64; then 64 alone cheaper, and 0 the alternative
    tie = np.full((3, 65), 100, np.uint8)
    tie[:, 0] = tie[:, 64] = 7
    got, rm, rr, ra, mg = check(f, tie, [0], [3], np.zeros((66, 66), np.uint8))
    assert got[0] == (0, 0, 0, 64) and ra[0, :3].tolist() == [64] * 3
    tie[:, 64] = 6
    got, rm, rr, ra, mg = check(f, tie, [0], [3], np.zeros((66, 66), np.uint8))
    assert got[0] == (1, 0, 64, 0) and rr[0, :3].tolist() == [64] * 3
    # INS of 64 behind 63 and of 63 behind 64 on random rows with those two cheap, the words overlapping
    rng = np.random.default_rng(13)
    rows = _rows(rng, 20)
    rows[:, 63] = rng.integers(0, 4, 20)
    rows[:, 64] = rng.integers(0, 4, 20)
    B = rng.integers(100, 256, (66, 66)).astype(np.uint8)
    B[63, 64] = B[64, 63] = B[65, 63] = B[65, 64] = B[63, 65] = B[64, 65] = 0
    first, n_of = _spans([20, 7, 1, 12])
    first[1:] = [0, 19, 4]
    got, rm, rr, ra, mg = check(f, rows, first, n_of, B, 2, 2)
    assert set(rr[0, :20].tolist()) <= {63, 64, 65}


def test_the_64_character_vector(f):
    C, B = insertion_vector()
    got, rm, rr, ra, mg = check(f, C, [0], [32], B, 1, 0)
    assert (rr[0] == 63).all() and got[0][0] > 0 and (mg[0, np.arange(32), 63] == 32).all()


def test_two_words_over_the_same_rows_and_a_repeat_call(S, f):
    rng = np.random.default_rng(14)
    costs = _rows(rng, 9)
    B = rng.integers(0, 40, (66, 66)).astype(np.uint8)
    got, rm, rr, ra, mg = check(f, costs, [0, 0], [9, 9], B, 30, 30)
    assert got[0] == got[1] and mg[0].tobytes() == mg[1].tobytes() and rm[0].tobytes() == rm[1].tobytes()
    host = S.word_margins_host(costs, [0, 0], [9, 9], B, 30, 30, want_marginals=True)
    assert WG.as_tuples(host[0]) == got and (host[1] == rm).all() and (host[2] == rr).all() and (host[3] == ra).all() and (host[4] == mg).all()


def test_errors_leave_the_context_usable(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    try:
        costs = np.zeros((2, 65), np.uint8)
        with pytest.raises(S.StrErError) as e:                           # no table
            ctx.word_margins(costs, [0], [2])
        assert e.value.code == -6 and "bigram" in str(e.value)
        ctx.set_bigram(np.zeros((66, 66), np.uint8))
        rec = ctx.word_margins(costs, [0, 0], [2, 0])[0]
        assert WG.as_tuples(rec) == [(0, 0, 0, 1), (-1, -1, -1, -1)]
        for first, n_of in (([1], [2]), ([0], [-1]), ([-1], [1])):
            with pytest.raises(S.StrErError) as e:                       # a word outside the cost rows
                ctx.word_margins(costs, first, n_of)
            assert e.value.code == -1
        assert ctx.word_margins(costs, [0, 0], [2, 0])[0].tobytes() == rec.tobytes()
    finally:
        ctx.close()
