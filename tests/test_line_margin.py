"""The line decoder's margins on the GPU (str_er_line_margins; the contract is at str_er_line_margin): every field of every record,
every per-row table and every marginal against the numpy reference (line_margin_ref.py) with ==, at the kernel's own edges -- the row
counts up to and past the limit of 1024, the lines of a workgroup (a wave each), the states 64 and 65 that live past the wave's 64
lanes, the largest values the bound of the contract allows -- and the identities of the contract against word_margins and
decode_lines of the same context."""
import numpy as np
import pytest

import line_decode_ref as LD
import line_margin_ref as LM
from test_line_decode_ref import _gaps, _rows, _spans, segmentation_gaps
from test_word_decode_ref import PAIRS

pytestmark = pytest.mark.gpu
LD_LINES = 4                      # lines of a workgroup of k_line_margin (LD_LINES, held against the header in test_line_decode.py)
NAMES = ("row_margin", "row_read", "row_alt", "gap_margin", "gap_move", "marginals")


@pytest.fixture(scope="module")
def f(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    yield ctx
    ctx.close()


def check(f, costs, gaps, first, n_of, B, ins=0, dele=0):
    """set_bigram, set_word_decode and line_margins (with the marginals) against the reference; returns the records as tuples and the
    reference's tables: row_margin, row_read, row_alt, gap_margin, gap_move, marginals."""
    f.set_bigram(B)
    f.set_word_decode(ins, dele)
    got = f.line_margins(costs, gaps, first, n_of, want_marginals=True)
    want = LM.line_margins(costs, gaps, first, n_of, B, ins, dele)
    recs = LM.as_tuples(got[0])
    assert recs == want[0], [(t, g, x) for t, (g, x) in enumerate(zip(recs, want[0])) if g != x][:5]
    for name, a, b in zip(NAMES, got[1:], want[1:]):
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), (name, np.argwhere(a != b)[:5])
    short = f.line_margins(costs, gaps, first, n_of)
    assert len(short) == 6 and all(a.tobytes() == b.tobytes() for a, b in zip(short, got))
    return (recs,) + tuple(want[1:])


@pytest.fixture(scope="module")
def row_count_case():
    rng = np.random.default_rng(1300)
    first, n_of = _spans([0, 1, 2, 31, 32, 33, 64, 65, 1023, 1024, 1025])
    n = int(n_of.sum())
    return first, n_of, _rows(rng, n), _gaps(rng, n, 8), rng.integers(0, 6, (66, 66)).astype(np.uint8)


@pytest.mark.parametrize("ins,dele", PAIRS)
def test_row_counts_under_every_pair_of_moves(f, row_count_case, ins, dele):
    first, n_of, costs, gaps, B = row_count_case
    recs, rm, rr, ra, gm, gv, mg = check(f, costs, gaps, first, n_of, B, ins, dele)
    assert recs[-1] == LM.NO_MARGIN and recs[0] == LM.NO_MARGIN               # 1025 rows: not decoded; no rows
    assert (rm[first[-1]:] == -1).all() and (rr[first[-1]:] == 0xFF).all() and (gv[first[-1]:] == 0xFF).all() and (mg[first[-1]:] == -1).all()
    for t, m in list(enumerate(n_of))[1:-1]:
        a = int(first[t])
        assert recs[t][0] >= 0 and (rm[a:a + m] >= 0).all() and gm[a] == -1 and gv[a] == 0xFF and (gv[a + 1:a + m] <= 1).all()
    assert int((gv == 1).sum()) > 100 and int((gv == 0).sum()) > 100 and int((gm > 0).sum()) > 100      # (the comparison does not stand on joins alone)


def test_the_bound_at_1024_rows(f):
    """Rows, table and gaps at their maxima: the dearest marginal there is, 1 043 202 < 2^20."""
    full, full_t = np.full((1024, 65), 255, np.uint8), np.full((66, 66), 255, np.uint8)
    G = np.full((1024, 2), 254, np.uint8)
    for ins, dele in ((255, 255), (0, 0)):
        G[:] = 254
        recs, rm, rr, ra, gm, gv, mg = check(f, full, G, [0], [1024], full_t, ins, dele)           # (254, 254): every gap has an alternative
        assert (gm[1:] >= 0).all()
        G[:] = (255, 254)
        recs, rm, rr, ra, gm, gv, mg = check(f, full, G, [0], [1024], full_t, ins, dele)
        assert (gm == -1).all() and (gv[1:] == 1).all() and recs[0][5:] == (-1, -1, -1)
        if (ins, dele) == (0, 0):
            assert mg.max() == 1043202
        G[:] = (254, 255)
        recs, rm, rr, ra, gm, gv, mg = check(f, full, G, [0], [1024], full_t, ins, dele)
        assert (gm == -1).all() and (gv[1:] == 0).all()


def test_line_counts_around_a_workgroup(S, f):
    rng = np.random.default_rng(1301)
    B = rng.integers(0, 6, (66, 66)).astype(np.uint8)
    for n in (0, 1, LD_LINES - 1, LD_LINES, LD_LINES + 1, 257):
        first, n_of = _spans(rng.integers(0, 12, n))
        rows = max(1, int(n_of.sum()))
        out = check(f, _rows(rng, rows), _gaps(rng, rows, 8), first, n_of, B, 20, 30)
        assert len(out[0]) == n and out[1].shape == (rows,) and out[6].shape == (rows, 68)
    got = f.line_margins(np.zeros((0, 65), np.uint8), np.zeros((0, 2), np.uint8), [], [], want_marginals=True)
    assert got[0].shape == (0,) and got[0].dtype == S.LINE_MARGIN_DTYPE and got[1].shape == (0,) and got[6].shape == (0, 68)
    got = f.line_margins(np.zeros((0, 65), np.uint8), np.zeros((0, 2), np.uint8), [0, 0], [0, 0])
    assert LM.as_tuples(got[0]) == [LM.NO_MARGIN] * 2


def test_paths_through_the_states_past_the_wave(f):
    zero = np.zeros((66, 66), np.uint8)
    # a line read as label 64 with the alternative 0, and the reverse
    rows = np.full((3, 65), 200, np.uint8)
    rows[:, 64], rows[:, 0] = 3, 5
    join = np.tile(np.array([0, 255], np.uint8), (3, 1))
    recs, rm, rr, ra, gm, gv, mg = check(f, rows, join, [0], [3], zero)
    assert rr.tolist() == [64] * 3 and ra.tolist() == [0] * 3 and rm.tolist() == [2] * 3 and recs[0] == (2, 2, 0, 64, 0, -1, -1, -1)
    rows[:, 64], rows[:, 0] = 5, 3
    recs, rm, rr, ra, gm, gv, mg = check(f, rows, join, [0], [3], zero)
    assert rr.tolist() == [0] * 3 and ra.tolist() == [64] * 3 and rm.tolist() == [2] * 3
    # a row whose alternative is 65: dropping it is the cheapest other thing to do
    recs, rm, rr, ra, gm, gv, mg = check(f, rows, join, [0], [3], zero, 0, 4)
    assert rr.tolist() == [0] * 3 and ra.tolist() == [65] * 3 and rm.tolist() == [1] * 3
    # the cases of the line decoder's test: label 64 with a blank after every second one; both moves on
    m = 6
    rows = np.full((m, 65), 200, np.uint8)
    rows[:, 64] = 3
    B = np.full((66, 66), 100, np.uint8)
    B[65, 64] = B[64, 64] = B[64, 65] = 1
    G = np.array([(0, 255), (0, 9), (9, 0), (0, 9), (9, 0), (0, 9)], np.uint8)
    recs, rm, rr, ra, gm, gv, mg = check(f, rows, G, [0], [m], B)
    assert rr.tolist() == [64] * m and gv.tolist() == [0xFF, 0, 1, 0, 1, 0] and (gm[1:] >= 0).all()
    # a break from state 64 with the join off: no alternative at that gap
    G[2] = (255, 7)
    recs, rm, rr, ra, gm, gv, mg = check(f, rows, G, [0], [m], B, 3, 4)
    assert gv[2] == 1 and gm[2] == -1 and mg[2, 66] == -1 and mg[2, 67] == mg[2, 64] and rr[1] == 64
    # a dropped row between two breaks: an empty word; the row reads 65
    rows3 = np.full((3, 65), 200, np.uint8)
    rows3[0, 64] = rows3[2, 64] = 0
    B3 = np.full((66, 66), 9, np.uint8)
    B3[65, 65] = 1
    recs, rm, rr, ra, gm, gv, mg = check(f, rows3, np.array([(0, 0), (255, 0), (255, 0)], np.uint8), [0], [3], B3, 0, 50)
    assert rr.tolist() == [64, 65, 64] and gv.tolist() == [0xFF, 1, 1] and mg[1, 65] == 9 + 9 + 50 + 1 + 9 + 9 and gm.tolist() == [-1, -1, -1]
    # ties between label 0 and label 64 (margin 0, the other label the alternative) and between a join and a break (the join is decided)
    tie = np.full((4, 65), 100, np.uint8)
    tie[:, 0] = tie[:, 64] = 7
    recs, rm, rr, ra, gm, gv, mg = check(f, tie, np.full((4, 2), 5, np.uint8), [0], [4], zero)
    assert rr.tolist() == [0] * 4 and ra.tolist() == [64] * 4 and rm.tolist() == [0] * 4
    assert gv.tolist() == [0xFF, 0, 0, 0] and gm.tolist() == [-1, 0, 0, 0] and recs[0] == (0, 0, 0, 0, 64, 0, 1, 0)
    tie[:, 0] = 8
    recs, rm, rr, ra, gm, gv, mg = check(f, tie, np.full((4, 2), 5, np.uint8), [0], [4], zero)
    assert rr.tolist() == [64] * 4 and ra.tolist() == [0] * 4 and rm.tolist() == [1] * 4


@pytest.mark.parametrize("ins,dele", PAIRS)
def test_identities_1_and_2_against_word_margins(f, ins, dele):
    rng = np.random.default_rng(1310 + ins + 7 * dele)
    lengths = [int(k) for k in rng.integers(1, 33, 24)] + [32, 1, 32]
    first, n_of = _spans(lengths)
    costs = _rows(rng, int(n_of.sum()))
    B = rng.integers(0, 256, (66, 66)).astype(np.uint8) if ins != 1 else rng.integers(0, 3, (66, 66)).astype(np.uint8)
    f.set_bigram(B)
    f.set_word_decode(ins, dele)
    wrec, wrm, wrr, wra, wmg = f.word_margins(costs, first, n_of, want_marginals=True)
    wcost = f.decode_words(costs, first, n_of)[0]["cost"].astype(np.int64)
    # (1) every word a line of its own, joins alone
    recs, rm, rr, ra, gm, gv, mg = check(f, costs, np.tile(np.array([0, 255], np.uint8), (len(costs), 1)), first, n_of, B, ins, dele)
    assert (gm == -1).all()
    for w, m in enumerate(lengths):
        a = int(first[w])
        assert (rm[a:a + m] == wrm[w, :m]).all() and (rr[a:a + m] == wrr[w, :m]).all() and (ra[a:a + m] == wra[w, :m]).all()
        assert (mg[a:a + m, :66] == wmg[w, :m]).all()
        assert recs[w] == (int(wrec[w]["margin"]), int(wrec[w]["margin"]), int(wrec[w]["row"]), int(wrec[w]["read"]), int(wrec[w]["alt"]), -1, -1, -1)
    # (2) all the words one line, its gaps forcing this segmentation: the marginals are the word's plus the other words' costs
    recs, rm, rr, ra, gm, gv, mg = check(f, costs, segmentation_gaps(lengths).astype(np.uint8), [0], [len(costs)], B, ins, dele)
    assert (gm == -1).all()
    for w, m in enumerate(lengths):
        a = int(first[w])
        assert (rm[a:a + m] == wrm[w, :m]).all() and (rr[a:a + m] == wrr[w, :m]).all() and (ra[a:a + m] == wra[w, :m]).all()
        assert (mg[a:a + m, :66] == np.where(wmg[w, :m] >= 0, wmg[w, :m] + int(wcost.sum() - wcost[w]), -1)).all()


@pytest.mark.parametrize("ins,dele", PAIRS)
def test_identity_3_against_decode_lines(f, ins, dele):
    """One line of 40 rows and, in one call, one copy of it per gap that has an alternative, the decided move of that gap off: every
    copy costs the line's cost plus the gap's margin."""
    rng = np.random.default_rng(1315 + ins + 7 * dele)
    m = 40
    C, G, B = _rows(rng, m), _gaps(rng, m, 8).astype(np.uint8), rng.integers(0, 6, (66, 66)).astype(np.uint8)
    recs, rm, rr, ra, gm, gv, mg = check(f, C, G, [0], [m], B, ins, dele)
    cost = int(f.decode_lines(C, G, [0], [m])[0][0]["cost"])
    at = [i for i in range(1, m) if gm[i] >= 0]
    assert len(at) >= 10
    gaps = np.tile(G, (len(at), 1))
    for k, i in enumerate(at):
        gaps[k * m + i, int(gv[i])] = 255
    first, n_of = _spans([m] * len(at))
    dec = f.decode_lines(np.tile(C, (len(at), 1)), gaps, first, n_of)[0]
    assert dec["cost"].tolist() == [cost + int(gm[i]) for i in at]


@pytest.fixture(scope="module")
def ground_case():
    rng = np.random.default_rng(1320)
    first, n_of = _spans(rng.integers(2, 40, 40))
    n = int(n_of.sum())
    return first, n_of, _rows(rng, n), rng.integers(0, 8, (n, 2)).astype(np.uint8), rng.integers(0, 6, (66, 66)).astype(np.uint8)


def test_the_ground_is_really_covered(f, ground_case):
    """Rows as test_word_margin._rows, gap bytes of integers(0, 8), a table of integers(0, 6), INS 20 and DEL 30: asserted on the
    reference, so that the comparison cannot pass on trivial cases, and the device agrees."""
    first, n_of, costs, gaps, B = ground_case
    recs, rm, rr, ra, gm, gv, mg = check(f, costs, gaps, first, n_of, B, 20, 30)
    n_gaps = int((n_of - 1).sum())
    assert int((gv == 1).sum()) >= n_gaps / 5 and int((gv == 0).sum()) >= n_gaps / 5, (int((gv == 1).sum()), n_gaps)
    assert int((gm == 0).sum()) >= 1 and int((gm > 0).sum()) >= 1
    assert int((rr == 65).sum()) >= 1 and int((ra == 65).sum()) >= 1 and int((rr == 64).sum()) >= 1
    by_gap = sum(1 for r in recs if r[5] >= 0 and r[0] == r[5] and r[5] < r[1])
    by_row = sum(1 for r in recs if r[0] == r[1] and (r[5] < 0 or r[1] < r[5]))
    assert by_gap >= 1 and by_row >= 1, (by_gap, by_row)


def test_two_calls_give_the_same_bytes(S, f):
    rng = np.random.default_rng(1330)
    first, n_of = _spans([70, 0, 200, 5])
    n = int(n_of.sum())
    costs, gaps, B = _rows(rng, n), _gaps(rng, n, 8), rng.integers(0, 40, (66, 66)).astype(np.uint8)
    f.set_bigram(B)
    f.set_word_decode(30, 30)
    a = f.line_margins(costs, gaps, first, n_of, want_marginals=True)
    b = f.line_margins(costs, gaps, first, n_of, want_marginals=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    host = S.line_margins_host(costs, gaps, first, n_of, B, 30, 30, want_marginals=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, host))
    assert f.line_margin_stats()["table_bytes"] >= 544 * n


def test_errors_leave_the_context_usable(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    try:
        costs, gaps = np.zeros((3, 65), np.uint8), np.zeros((3, 2), np.uint8)
        assert ctx.line_margin_stats()["table_bytes"] == 0
        with pytest.raises(S.StrErError) as e:                           # no table
            ctx.line_margins(costs, gaps, [0], [3])
        assert e.value.code == -6 and "bigram" in str(e.value)
        ctx.set_bigram(np.zeros((66, 66), np.uint8))
        ok = ctx.line_margins(costs, gaps, [0, 3], [3, 0])
        assert LM.as_tuples(ok[0]) == [(0, 0, 0, 0, 1, 0, 1, 0), LM.NO_MARGIN]      # (all zeros: every row and every gap ties)
        for first, n_of in (([1], [3]), ([0], [-1]), ([-1], [1]), ([0, 2], [3, 1]), ([2, 0], [1, 2])):
            with pytest.raises(S.StrErError) as e:                       # a window outside the rows, over another or out of order
                ctx.line_margins(costs, gaps, first, n_of)
            assert e.value.code == -1
        bad = gaps.copy()
        bad[1] = 255
        with pytest.raises(S.StrErError) as e:                           # both moves off at a gap
            ctx.line_margins(costs, bad, [0], [3])
        assert e.value.code == -1 and "both moves off" in str(e.value)
        bad[1], bad[0] = 0, 255                                          # (the pair of a line's first row is ignored)
        assert ctx.line_margins(costs, bad, [0, 3], [3, 0])[0].tobytes() == ok[0].tobytes()
        ctx.set_line_margin(True)
        ctx.set_line_margin(False)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ctx.line_margins(costs, gaps, [0, 3], [3, 0]), ok))
        assert LD.as_tuples(ctx.decode_lines(costs, gaps, [0, 3], [3, 0])[0]) == [(0, 3, 0, 3, 0, 0), (0, 0, 0, 0, 0, 0)]
    finally:
        ctx.close()
