"""The numpy reference of the line decoder's margins (line_margin_ref.py, written from the definition at str_er_line_margin) against an
enumeration of every path on alphabets of 2 and 3 characters, the three identities of the contract on the reference at the library's
alphabet against the word margins' reference (word_margin_ref.py) and the line decoder's (line_decode_ref.py), and the pure host entry
point -- str_er_line_margins_host -- against the reference, every value with ==."""
import numpy as np
import pytest

import line_decode_ref as LD
import line_margin_ref as LM
import word_margin_ref as WM
from test_line_decode_ref import _gaps, _rows, _spans, segmentation_gaps
from test_word_decode_ref import PAIRS


@pytest.mark.parametrize("n,ms,reps", ((2, (1, 2, 3, 4), 8), (3, (1, 2, 3, 4), 5)))
def test_reference_equals_the_enumeration_of_every_path(n, ms, reps):
    rng = np.random.default_rng(1300 + n)
    for m in ms:
        for ins, dele in PAIRS:
            for rep in range(reps if m < 4 else 2 if n == 2 else 1):      # (4 rows of 3 characters with INS: a second a case)
                hi = (4, 16, 256)[(rep + ins) % 3]              # small ranges tie often
                C = rng.integers(0, hi, (m, n))
                B = rng.integers(0, hi, (n + 1, n + 1))
                G = _gaps(rng, m, min(hi, 255))                 # (off moves on either side)
                cost, M, MG = LM.marginals_backward(C, G, B, ins, dele, n)
                best, Me, MGe = LM.marginals_enumerated(C, G, B, ins, dele, n)
                assert cost == best and (M == Me).all() and (MG == MGe).all(), (m, ins, dele, C, G, B)
                assert all(min(v for v in M[i] if v >= 0) == cost for i in range(m))
                assert all(min(v for v in MG[i] if v >= 0) == cost for i in range(1, m)) and (MG[0] == -1).all()
                # the readings attain cost (asserted inside), the margins are >= 0, the record is the smallest of them
                rec, rm, rr, ra, gm, gv, mg, c2 = LM.margins_line(C, G, B, ins, dele, n)
                assert c2 == cost and min(rm) >= 0 and all(g >= -1 for g in gm) and gm[0] == -1 and gv[0] == -1
                assert rec[1] == min(rm) and rec[0] == min([rec[1]] + [g for g in gm if g >= 0])
                for i in range(1, m):
                    assert (gm[i] == -1) == (int(G[i, 1 - gv[i]]) == 255)


def test_the_three_character_alphabet_at_four_rows():
    rng = np.random.default_rng(1304)
    for dele in (0, 3):
        C, B, G = rng.integers(0, 6, (4, 3)), rng.integers(0, 6, (4, 4)), _gaps(rng, 4, 6)
        cost, M, MG = LM.marginals_backward(C, G, B, 0, dele, 3)
        best, Me, MGe = LM.marginals_enumerated(C, G, B, 0, dele, 3)
        assert cost == best and (M == Me).all() and (MG == MGe).all()


@pytest.mark.parametrize("ins,dele", PAIRS)
def test_identity_1_joins_alone_are_the_word_margins(ins, dele):
    rng = np.random.default_rng(1310 + ins + 7 * dele)
    for m in (1, 2, 7, 32):
        for hi in (6, 256):
            C, B = _rows(rng, m), rng.integers(0, hi, (66, 66))
            rec, rm, rr, ra, gm, gv, mg, cost = LM.margins_line(C, np.tile([0, 255], (m, 1)), B, ins, dele)
            wrec, wrm, wrr, wra, wM, wcost = WM.margins_word(C, B, ins, dele)
            assert cost == wcost and rm == wrm and rr == wrr and ra == wra and (mg[:, :66] == wM).all()
            assert gm == [-1] * m and rec == (wrec[0], wrec[0], wrec[1], wrec[2], wrec[3], -1, -1, -1)
            assert (mg[1:, 66] == cost).all() and (mg[:, 67] == -1).all() and mg[0, 66] == -1


@pytest.mark.parametrize("ins,dele", PAIRS)
def test_identity_2_a_forced_segmentation_is_its_words(ins, dele):
    rng = np.random.default_rng(1320 + ins + 7 * dele)
    for rep in range(8):
        lengths = [int(k) for k in rng.integers(1, 9, int(rng.integers(1, 6)))]
        C = _rows(rng, sum(lengths))
        B = rng.integers(0, (6, 64, 256)[rep % 3], (66, 66))
        rec, rm, rr, ra, gm, gv, mg, cost = LM.margins_line(C, segmentation_gaps(lengths), B, ins, dele)
        words = []
        at = 0
        for k in lengths:
            words.append(WM.margins_word(C[at:at + k], B, ins, dele))
            at += k
        assert cost == sum(w[5] for w in words) and gm == [-1] * len(C)
        at = 0
        for w, k in zip(words, lengths):
            assert rm[at:at + k] == w[1] and rr[at:at + k] == w[2] and ra[at:at + k] == w[3]
            others = cost - w[5]
            assert (mg[at:at + k, :66] == np.where(w[4] >= 0, w[4] + others, -1)).all()
            at += k
        assert gv == [-1] + [1 if i in set(np.cumsum(lengths)[:-1].tolist()) else 0 for i in range(1, len(C))]


@pytest.mark.parametrize("ins,dele", PAIRS)
def test_identity_3_a_gap_margin_is_the_price_of_the_other_move(ins, dele):
    rng = np.random.default_rng(1330 + ins + 7 * dele)
    n_checked = 0
    for rep in range(4):
        m = int(rng.integers(2, 14))
        C, G, B = _rows(rng, m), _gaps(rng, m, (8, 255)[rep % 2]), rng.integers(0, (6, 256)[rep % 2], (66, 66))
        rec, rm, rr, ra, gm, gv, mg, cost = LM.margins_line(C, G, B, ins, dele)
        for i in range(1, m):
            if gm[i] < 0:
                continue
            G2 = G.copy()
            G2[i, gv[i]] = 255
            assert LD.decode_line(C, G2, B, ins, dele)[0][0] == cost + gm[i]
            n_checked += 1
    assert n_checked >= 4


def test_not_decoded_past_1024_rows_and_the_bound_at_1024():
    full_rows, full_t = np.full((1025, 65), 255, np.uint8), np.full((66, 66), 255, np.uint8)
    G = np.full((1025, 2), 254, np.uint8)
    assert LM.margins_line(full_rows, G, full_t)[0] == LM.NO_MARGIN and LM.margins_line(full_rows[:0], G[:0], full_t)[0] == LM.NO_MARGIN
    G[:, 0] = 255
    rec, rm, rr, ra, gm, gv, mg, cost = LM.margins_line(full_rows[:1024], G[:1024], full_t, 0, 0)
    assert cost == 1043202 and mg.max() == 1043202 < LM.INF and rec == (0, 0, 0, 0, 1, -1, -1, -1) and set(gv[1:]) == {1}


# ---- the host entry point -----------------------------------------------------------------------------------------------------------

def check_host(S, costs, gaps, first, n_of, B, ins, dele):
    got = S.line_margins_host(costs, gaps, first, n_of, B, ins, dele, want_marginals=True)
    want = LM.line_margins(costs, gaps, first, n_of, B, ins, dele)
    assert got[0].dtype == S.LINE_MARGIN_DTYPE and [a.dtype for a in got[1:]] == [np.int32, np.uint8, np.uint8, np.int32, np.uint8, np.int32]
    assert LM.as_tuples(got[0]) == want[0]
    for a, b in zip(got[1:], want[1:]):
        assert a.shape == b.shape and (a == b).all()
    short = S.line_margins_host(costs, gaps, first, n_of, B, ins, dele)
    assert len(short) == 6 and all((a == b).all() for a, b in zip(short, got))
    return want


@pytest.mark.parametrize("ins,dele", PAIRS)
def test_line_margins_host_equals_the_reference(S, ins, dele):
    rng = np.random.default_rng(1340 + ins + 7 * dele)
    first, n_of = _spans([0, 1, 2, 31, 32, 33, 64, 65] + list(rng.integers(0, 13, 8)))
    first[1:] += 2                                               # (two rows of no line in front of the second line)
    n = int(first[-1] + n_of[-1]) + 3
    costs, gaps = _rows(rng, n), _gaps(rng, n)
    for hi in (6, 256):
        want = check_host(S, costs, gaps, first, n_of, rng.integers(0, hi, (66, 66)).astype(np.uint8), ins, dele)
    assert want[0][0] == LM.NO_MARGIN and (want[1][:2] == -1).all() and (want[5][-3:] == 0xFF).all() and (want[6][-3:] == -1).all()


def test_line_margins_host_at_the_row_limit(S):
    rng = np.random.default_rng(1350)
    first, n_of = _spans([1023, 1024, 1025])
    n = int(n_of.sum())
    costs, gaps = _rows(rng, n), _gaps(rng, n, 8)
    want = check_host(S, costs, gaps, first, n_of, rng.integers(0, 6, (66, 66)).astype(np.uint8), 20, 30)
    assert want[0][2] == LM.NO_MARGIN and want[0][1][0] >= 0 and (want[1][2047:] == -1).all()
    full = np.full((1024, 65), 255, np.uint8)
    G = np.full((1024, 2), 254, np.uint8)
    G[:, 0] = 255
    want = check_host(S, full, G, [0], [1024], np.full((66, 66), 255, np.uint8), 0, 0)
    assert want[6].max() == 1043202
    got = S.line_margins_host(costs, gaps, [], [], np.zeros((66, 66), np.uint8), want_marginals=True)
    assert got[0].shape == (0,) and (got[1] == -1).all() and (got[2] == 0xFF).all() and (got[6] == -1).all()
