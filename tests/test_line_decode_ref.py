"""The numpy reference of the line decoder (line_decode_ref.py, written from the definition at str_er_line_decode) against an
enumeration of every path on alphabets of 2 and 3 characters, the three identities of the contract against the word decoder's
reference (word_decode_ref.py), and the pure host entry points -- str_er_decode_lines_host, str_er_line_gap_costs -- against the
reference, every value with ==."""
import numpy as np
import pytest

import line_decode_ref as LD
import word_decode_ref as WD
from test_word_decode_ref import PAIRS


def _rows(rng, n):
    """Random cost rows: a few cheap characters per run among dear ones (as test_word_margin._rows)."""
    c = rng.integers(60, 256, (n, 65))
    cheap = rng.random((n, 65)) < 0.08
    c[cheap] = rng.integers(0, 24, int(cheap.sum()))
    return c.astype(np.uint8)


def _gaps(rng, m, hi=255):
    """Random gap pairs below hi <= 255, some moves off, never both."""
    G = rng.integers(0, hi, (m, 2))
    off = rng.integers(0, 6, m)
    G[off == 0, 0] = 255
    G[off == 1, 1] = 255
    return G


def segmentation_gaps(lengths, join=(0, 255), brk=(255, 0)):
    """The gap pairs that force a segmentation into words of these lengths."""
    G = []
    for k in lengths:
        G += [brk] + [join] * (k - 1) if k else []
    return np.array(G, np.int64).reshape(-1, 2)


def words_of_segmentation(C, lengths, B, ins, dele, n=65):
    """(the sum of the words' decoder costs, their labels joined by one blank) under word_decode_ref."""
    at, total, labels = 0, 0, []
    for w, k in enumerate(lengths):
        rec, lab, src = WD.decode_word(C[at:at + k], B, ins, dele, n)
        total += rec[0]
        labels += ([n] if w else []) + lab
        at += k
    return total, labels


@pytest.mark.parametrize("n,ms,reps", ((2, (0, 1, 2, 3, 4), 8), (3, (0, 1, 2, 3), 5)))
def test_reference_equals_the_enumeration_of_every_path(n, ms, reps):
    rng = np.random.default_rng(300 + n)
    for m in ms:
        for ins, dele in PAIRS:
            for rep in range(reps if m < 4 else 2):
                hi = (4, 16, 256)[rep % 3]                      # small ranges tie often
                C = rng.integers(0, hi, (m, n))
                B = rng.integers(0, hi, (n + 1, n + 1))
                G = _gaps(rng, m, min(hi, 255))
                rec, lab, src, wor = LD.decode_line(C, G, B, ins, dele, n)
                assert rec[0] == LD.enumerate_best(C, G, B, ins, dele, n), (m, ins, dele, C, G, B)
                assert rec[0] == LD.path_cost(C, G, B, lab, src, ins, dele, n)
                assert rec[3] + rec[5] + rec[2] == rec[1] == len(lab) <= max(0, 3 * m - 1) and rec[3] + rec[4] == m
                assert lab.count(n) == rec[2] and (ins > 0 or rec[5] == 0) and (dele > 0 or rec[4] == 0)
                assert [w for w in wor if w >= 0] == sorted(w for w in wor if w >= 0) and wor.count(-1) == rec[4] and max(wor, default=0) <= rec[2]


def test_the_three_character_alphabet_at_four_rows():
    rng = np.random.default_rng(304)
    for dele in (0, 3):
        C, B, G = rng.integers(0, 6, (4, 3)), rng.integers(0, 6, (4, 4)), _gaps(rng, 4, 6)
        assert LD.decode_line(C, G, B, 0, dele, 3)[0][0] == LD.enumerate_best(C, G, B, 0, dele, 3)


@pytest.mark.parametrize("ins,dele", PAIRS)
def test_identity_1_joins_alone_are_the_word_decoder(ins, dele):
    rng = np.random.default_rng(310 + ins + 7 * dele)
    for m in (0, 1, 2, 7, 32):
        for hi in (6, 256):
            C, B = _rows(rng, m), rng.integers(0, hi, (66, 66))
            rec, lab, src, wor = LD.decode_line(C, np.tile([0, 255], (m, 1)), B, ins, dele)
            want, wlab, wsrc = WD.decode_word(C, B, ins, dele)
            assert rec[0] == want[0] and rec[2] == 0 and (rec[1], rec[3], rec[4], rec[5]) == want[2:]
            assert lab == wlab and src == [(s & 0x7F) | (0x8000 if s & 0x80 else 0) for s in wsrc]


@pytest.mark.parametrize("ins,dele", PAIRS)
def test_identities_2_and_3_against_the_words_of_a_segmentation(ins, dele):
    rng = np.random.default_rng(320 + ins + 7 * dele)
    for rep in range(12):
        lengths = [int(k) for k in rng.integers(1, 9, int(rng.integers(1, 6)))]
        m = sum(lengths)
        C = _rows(rng, m)
        B = rng.integers(0, (6, 64, 256)[rep % 3], (66, 66))             # (B[E][E] != 0 almost always)
        total, labels = words_of_segmentation(C, lengths, B, ins, dele)
        rec, lab, src, wor = LD.decode_line(C, segmentation_gaps(lengths), B, ins, dele)
        assert rec[0] == total and lab == labels and rec[2] == len(lengths) - 1
        # (3) both moves on everywhere: never worse than the segmentation with what it pays at its gaps
        G = rng.integers(0, 255, (m, 2))
        starts = set(np.cumsum(lengths)[:-1].tolist())
        paid = sum(int(G[i, 1]) if i in starts else int(G[i, 0]) for i in range(1, m))
        rec3 = LD.decode_line(C, G, B, ins, dele)[0]
        assert rec3[0] <= total + paid


def test_breaks_and_empty_words_are_really_taken():
    """The ground the device comparison stands on: with a table of integers(0, 6) the reference breaks at between 1/5 and 4/5 of the
    gaps, and with integers(0, 256) empty words occur."""
    rng = np.random.default_rng(330)
    n_gaps = n_breaks = n_empty = 0
    for t in range(40):
        m = int(rng.integers(2, 40))
        C, G = _rows(rng, m), rng.integers(0, 255, (m, 2))
        rec, lab, src, wor = LD.decode_line(C, G, rng.integers(0, 6, (66, 66)), 20, 30)
        n_gaps += m - 1
        n_breaks += rec[2]
        rec, lab, src, wor = LD.decode_line(C, G, rng.integers(0, 256, (66, 66)), 20, 30)
        n_empty += rec[2] + 1 - len(set(w for w in wor if w >= 0))
    assert 0.2 * n_gaps <= n_breaks <= 0.8 * n_gaps, (n_breaks, n_gaps)
    assert n_empty >= 1


def test_not_decoded_past_1024_rows_and_the_bound_at_1024():
    full_rows, full_t = np.full((1025, 65), 255, np.uint8), np.full((66, 66), 255, np.uint8)
    G = np.full((1025, 2), 254, np.uint8)
    rec, lab, src, wor = LD.decode_line(full_rows, G, full_t, 0, 0)
    assert rec == (-1, 0, 0, 0, 0, 0) and lab == [] and wor == [-1] * 1025
    rec, lab, src, wor = LD.decode_line(full_rows[:1024], G[:1024], full_t, 0, 0)
    assert rec[0] == 510 + (255 + 255 + 254) * 1023 + 255 < 1043202 < LD.INF and rec[2] == 0        # (a join is the cheaper move at every gap)
    G[:, 0] = 255
    rec, lab, src, wor = LD.decode_line(full_rows[:1024], G[:1024], full_t, 0, 0)
    assert rec[0] == 1043202 and rec[2] == 1023 and rec[1] == 2047


# ---- the host entry points ----------------------------------------------------------------------------------------------------------

def _spans(n_of):
    n_of = np.asarray(n_of, np.int64)
    return np.concatenate([[0], np.cumsum(n_of)])[:len(n_of)].astype(np.int32), n_of.astype(np.int32)


def check_host(S, costs, gaps, first, n_of, B, ins, dele):
    dec, chars, src, wor = S.decode_lines_host(costs, gaps, first, n_of, B, ins, dele)
    want = LD.decode_lines(costs, gaps, first, n_of, B, ins, dele)
    assert dec.dtype == S.LINE_DECODE_DTYPE and chars.dtype == np.uint8 and src.dtype == np.uint16 and wor.dtype == np.int32
    assert LD.as_tuples(dec) == want[0]
    assert (chars == want[1]).all() and (src == want[2]).all() and (wor == want[3]).all()
    return want


@pytest.mark.parametrize("ins,dele", PAIRS)
def test_decode_lines_host_equals_the_reference(S, ins, dele):
    rng = np.random.default_rng(340 + ins + 7 * dele)
    first, n_of = _spans([0, 1, 2, 31, 32, 33, 64, 65] + list(rng.integers(0, 13, 8)))
    first[1:] += 2                                               # (two rows of no line in front of the second line)
    n = int(first[-1] + n_of[-1]) + 3
    costs, gaps = _rows(rng, n), _gaps(rng, n)
    for hi in (6, 256):
        want = check_host(S, costs, gaps, first, n_of, rng.integers(0, hi, (66, 66)).astype(np.uint8), ins, dele)
    assert (want[1][:6] == 0xFF).all() and (want[3][-3:] == -1).all()


def test_decode_lines_host_at_the_row_limit(S):
    rng = np.random.default_rng(350)
    first, n_of = _spans([1023, 1024, 1025])
    n = int(n_of.sum())
    costs, gaps = _rows(rng, n), _gaps(rng, n)
    want = check_host(S, costs, gaps, first, n_of, rng.integers(0, 6, (66, 66)).astype(np.uint8), 20, 30)
    assert want[0][2] == (-1, 0, 0, 0, 0, 0) and want[0][1][0] >= 0
    full = np.full((1024, 65), 255, np.uint8)
    G = np.full((1024, 2), 254, np.uint8)
    G[:, 0] = 255
    want = check_host(S, full, G, [0], [1024], np.full((66, 66), 255, np.uint8), 0, 0)
    assert want[0][0][0] == 1043202
    dec, chars, src, wor = S.decode_lines_host(costs, gaps, [], [], np.zeros((66, 66), np.uint8))
    assert dec.shape == (0,) and (chars == 0xFF).all() and (wor == -1).all()


def test_line_gap_costs_equals_the_reference_and_its_corners(S):
    rng = np.random.default_rng(360)
    for rep in range(20):
        n_lines = int(rng.integers(1, 6))
        n_of = rng.integers(0, 9, n_lines)
        first, n_of = _spans(n_of)
        n = int(n_of.sum())
        runs = np.zeros(n, S.LINE_RUN_DTYPE)
        x = 0
        for r in range(n):
            w, g = int(rng.integers(1, 30)), int(rng.integers(1, 60))
            runs[r]["x0"], runs[r]["x1"] = x + g, x + g + w
            x += g + w
        colmax = rng.integers(1, 60, n_lines)
        num, den, w = int(rng.integers(1, 5)), int(rng.integers(1, 7)), int(rng.integers(0, 128))
        got = S.line_gap_costs(runs, first, n_of, colmax, num, den, w)
        want = LD.gap_costs([(int(q["x0"]), int(q["x1"])) for q in runs], first, n_of, colmax, num, den, w)
        assert got.shape == (n, 2) and (got == want).all(), (rep, got, want)
        assert (got[:, 0].astype(int) <= 254).all() or n == 0
    # the corners at 1 / 3 and colmax 9: the threshold is g = 3 (3 g >= 9): there J == K; one below, the join is cheaper; far above, J = 2 w and K = 0
    def pair(g, colmax=9, w=16, num=1, den=3):
        runs = np.zeros(2, S.LINE_RUN_DTYPE)
        runs["x0"], runs["x1"] = [10, 20 + g], [20, 25 + g]
        got = S.line_gap_costs(runs, [0], [2], [colmax], num, den, w)
        assert tuple(got[0]) == (0, 255)
        assert tuple(int(v) for v in got[1]) == LD.gap_pair(g, colmax, num, den, w)
        return tuple(int(v) for v in got[1])
    assert pair(3) == (16, 16) and pair(2) == (10, 22) and pair(1000) == (32, 0) and pair(6) == (32, 0) and pair(5) == (26, 6)
    assert pair(3, w=0) == (0, 0) and pair(1000, w=0) == (0, 0)
    assert pair(3, w=127) == (127, 127) and pair(1000, w=127) == (254, 0) and pair(0, w=127) == (0, 254)
    assert pair(1, colmax=1) == (32, 0) and pair(1, colmax=1, num=65535, den=1) == (0, 32) and pair(1, colmax=16384, num=1, den=65535) == (32, 0)
    # rows of the same run (the parts of a split run) get (0, 255); a row of no line too
    runs = np.zeros(2, S.LINE_RUN_DTYPE)
    runs["x0"], runs["x1"] = [10, 40], [20, 50]
    got = S.line_gap_costs(runs, [1], [4], [9], 1, 3, 16, row_run=[0, 0, 0, 1, 1, 1])
    assert got.tolist() == [[0, 255], [0, 255], [0, 255], [32, 0], [0, 255], [0, 255]]
    want = LD.gap_costs([(10, 20), (40, 50)], [1], [4], [9], 1, 3, 16, row_run=[0, 0, 0, 1, 1, 1])
    assert (got == want).all()
