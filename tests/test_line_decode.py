"""The line decoder on the GPU (str_er_decode_lines; the contract is at str_er_line_decode): every field of every record, every label,
source and word of a row against the numpy reference (line_decode_ref.py) with ==, at the kernel's own edges -- the row counts up to
and past the limit of 1024 and around the 64-entry chunks of the move to the front, the lines of a workgroup (a wave each), the
states 64 and 65 that live past the wave's 64 lanes, the largest values the bound of the contract allows -- and the identities of
the contract against decode_words of the same context."""
import os
import re

import numpy as np
import pytest

import line_decode_ref as LD
from test_line_decode_ref import _gaps, _rows, _spans, segmentation_gaps
from test_word_decode_ref import PAIRS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD_LINES = 4                      # lines of a workgroup of k_line_decode (LD_LINES)


@pytest.fixture(scope="module")
def f(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    yield ctx
    ctx.close()


def check(f, costs, gaps, first, n_of, B, ins=0, dele=0):
    """set_bigram, set_word_decode and decode_lines against the reference; returns the records as tuples, chars, src, word_of_row."""
    f.set_bigram(B)
    f.set_word_decode(ins, dele)
    dec, chars, src, wor = f.decode_lines(costs, gaps, first, n_of)
    want = LD.decode_lines(costs, gaps, first, n_of, B, ins, dele)
    got = LD.as_tuples(dec)
    assert got == want[0], [(t, g, x) for t, (g, x) in enumerate(zip(got, want[0])) if g != x][:5]
    assert (chars == want[1]).all() and (src == want[2]).all() and (wor == want[3]).all(), (np.argwhere(chars != want[1])[:5], np.argwhere(src != want[2])[:5],
                                                                                              np.argwhere(wor != want[3])[:5])
    return got, chars, src, wor


def test_the_lines_of_a_workgroup_are_the_header_s():
    with open(os.path.join(ROOT, "scene-text-recognition_amd", "csrc", "line_decode_kernels.h")) as h:
        assert int(re.search(r"constexpr int LD_LINES = (\d+);", h.read()).group(1)) == LD_LINES


@pytest.fixture(scope="module")
def row_count_case():
    rng = np.random.default_rng(1200)
    first, n_of = _spans([0, 1, 2, 31, 32, 33, 64, 65, 1023, 1024, 1025])
    n = int(n_of.sum())
    return first, n_of, _rows(rng, n), _gaps(rng, n), rng.integers(0, 6, (66, 66)).astype(np.uint8)


@pytest.mark.parametrize("ins,dele", PAIRS)
def test_row_counts_under_every_pair_of_moves(f, row_count_case, ins, dele):
    first, n_of, costs, gaps, B = row_count_case
    got, chars, src, wor = check(f, costs, gaps, first, n_of, B, ins, dele)
    assert got[-1] == (-1, 0, 0, 0, 0, 0)                                  # 1025 rows: not decoded
    assert (chars[3 * first[-1]:] == 0xFF).all() and (src[3 * first[-1]:] == 0xFFFF).all() and (wor[first[-1]:] == -1).all()
    assert got[0] == (int(B[65, 65]), 0, 0, 0, 0, 0)                        # no rows
    for t, m in list(enumerate(n_of))[1:-1]:
        cost, n_chars, n_brk, n_sub, n_del, n_ins = got[t]
        assert cost >= 0 and n_sub + n_ins + n_brk == n_chars <= 3 * m - 1 and n_sub + n_del == m and n_brk <= m - 1
        lab = chars[3 * first[t]:3 * first[t] + 3 * m]
        assert (lab[:n_chars] <= 65).all() and (lab[n_chars:] == 0xFF).all() and int((lab[:n_chars] == 65).sum()) == n_brk
    assert sum(g[2] for g in got) > 100                                     # (the comparison does not stand on joins alone)


def test_the_bound_at_1024_rows(f):
    """Rows, table and gaps at their maxima: the dearest line there is, 510 + 1019 * 1023 + 255 = 1 043 202 < 2^20."""
    full, full_t = np.full((1024, 65), 255, np.uint8), np.full((66, 66), 255, np.uint8)
    G = np.full((1024, 2), 254, np.uint8)
    got, chars, src, wor = check(f, full, G, [0], [1024], full_t)
    assert got[0][0] == 510 + 764 * 1023 + 255 and got[0][2] == 0
    G[:, 0] = 255
    got, chars, src, wor = check(f, full, G, [0], [1024], full_t)
    assert got[0] == (1043202, 2047, 1023, 1024, 0, 0) and wor[-1] == 1023 and src[2046] == 1023 and src[2045] == 1023 | 0x4000
    check(f, full, G, [0], [1024], full_t, 255, 255)
    G[:] = (254, 255)
    check(f, full, G, [0], [1024], full_t, 255, 255)


def test_line_counts_around_a_workgroup(S, f):
    rng = np.random.default_rng(1201)
    B = rng.integers(0, 6, (66, 66)).astype(np.uint8)
    for n in (0, 1, LD_LINES - 1, LD_LINES, LD_LINES + 1, 257):
        first, n_of = _spans(rng.integers(0, 12, n))
        rows = max(1, int(n_of.sum()))
        got, chars, src, wor = check(f, _rows(rng, rows), _gaps(rng, rows), first, n_of, B, 20, 30)
        assert len(got) == n and chars.shape == (3 * rows,) and src.shape == (3 * rows,) and wor.shape == (rows,)
    dec, chars, src, wor = f.decode_lines(np.zeros((0, 65), np.uint8), np.zeros((0, 2), np.uint8), [], [])
    assert dec.shape == (0,) and dec.dtype == S.LINE_DECODE_DTYPE and chars.shape == (0,) and wor.shape == (0,)
    dec, chars, src, wor = f.decode_lines(np.zeros((0, 65), np.uint8), np.zeros((0, 2), np.uint8), [0, 0], [0, 0])
    assert LD.as_tuples(dec) == [(int(B[65, 65]), 0, 0, 0, 0, 0)] * 2


def test_paths_through_the_states_past_the_wave(f):
    # a line whose cheapest characters are label 64, with a blank after every second one
    m = 6
    rows = np.full((m, 65), 200, np.uint8)
    rows[:, 64] = 3
    B = np.full((66, 66), 100, np.uint8)
    B[65, 64] = B[64, 64] = B[64, 65] = 1
    G = np.array([(0, 255), (0, 9), (9, 0), (0, 9), (9, 0), (0, 9)], np.uint8)
    got, chars, src, wor = check(f, rows, G, [0], [m], B)
    assert chars[:8].tolist() == [64, 64, 65, 64, 64, 65, 64, 64] and wor.tolist() == [0, 0, 1, 1, 2, 2]
    assert src[:8].tolist() == [0, 1, 2 | 0x4000, 2, 3, 4 | 0x4000, 4, 5]
    # a line that must break from state 64: the join is off
    G[2] = (255, 7)
    got, chars, src, wor = check(f, rows, G, [0], [m], B, 3, 4)
    assert chars[2] == 65 and chars[1] == 64
    # a dropped row between two breaks: an empty word, which pays B[E][E]
    rows3 = np.full((3, 65), 200, np.uint8)
    rows3[0, 64] = rows3[2, 64] = 0
    B3 = np.full((66, 66), 9, np.uint8)
    B3[65, 65] = 1
    got, chars, src, wor = check(f, rows3, np.array([(0, 0), (255, 0), (255, 0)], np.uint8), [0], [3], B3, 0, 50)
    assert got[0] == (9 + 9 + 50 + 1 + 9 + 9, 4, 2, 2, 1, 0) and chars[:4].tolist() == [64, 65, 65, 64] and wor.tolist() == [0, -1, 2]
    # ties between label 0 and label 64, and between a join and a break: the smallest state, and the join
    tie = np.full((4, 65), 100, np.uint8)
    tie[:, 0] = tie[:, 64] = 7
    got, chars, src, wor = check(f, tie, np.full((4, 2), 5, np.uint8), [0], [4], np.zeros((66, 66), np.uint8))
    assert got[0][2] == 0 and chars[:4].tolist() == [0] * 4
    tie[:, 0] = 8
    got, chars, src, wor = check(f, tie, np.full((4, 2), 5, np.uint8), [0], [4], np.zeros((66, 66), np.uint8))
    assert got[0][2] == 0 and chars[:4].tolist() == [64] * 4


@pytest.mark.parametrize("ins,dele", PAIRS)
def test_identities_1_and_2_against_decode_words(f, ins, dele):
    rng = np.random.default_rng(1210 + ins + 7 * dele)
    lengths = [int(k) for k in rng.integers(1, 33, 24)] + [32, 1, 32]
    first, n_of = _spans(lengths)
    costs = _rows(rng, int(n_of.sum()))
    B = rng.integers(0, 256, (66, 66)).astype(np.uint8) if ins != 1 else rng.integers(0, 3, (66, 66)).astype(np.uint8)
    f.set_bigram(B)
    f.set_word_decode(ins, dele)
    wdec, wchars, wsrc = f.decode_words(costs, first, n_of)
    # (1) every word a line of its own, joins alone
    got, chars, src, wor = check(f, costs, np.tile(np.array([0, 255], np.uint8), (len(costs), 1)), first, n_of, B, ins, dele)
    for w, m in enumerate(lengths):
        n_chars = int(wdec[w]["n_chars"])
        assert got[w] == (int(wdec[w]["cost"]), n_chars, 0, int(wdec[w]["n_sub"]), int(wdec[w]["n_del"]), int(wdec[w]["n_ins"]))
        assert (chars[3 * first[w]:3 * first[w] + n_chars] == wchars[w, :n_chars]).all()
        s = wsrc[w, :n_chars].astype(np.uint16)
        assert (src[3 * first[w]:3 * first[w] + n_chars] == ((s & 0x7F) | ((s & 0x80) << 8))).all()
    # (2) all the words one line, its gaps forcing this segmentation
    got, chars, src, wor = check(f, costs, segmentation_gaps(lengths).astype(np.uint8), [0], [len(costs)], B, ins, dele)
    assert got[0][0] == int(wdec["cost"].sum()) and got[0][2] == len(lengths) - 1
    want = []
    for w in range(len(lengths)):
        want += ([65] if w else []) + wchars[w, :int(wdec[w]["n_chars"])].tolist()
    assert chars[:got[0][1]].tolist() == want


def test_the_ground_is_really_covered(f):
    """Rows as test_word_margin._rows and gap bytes of integers(0, 255): with a table of integers(0, 6) the reference breaks at between
    1/5 and 4/5 of the gaps, with integers(0, 256) it makes empty words -- asserted on the reference, so that the comparison above cannot
    pass on joins alone -- and the device agrees on both."""
    rng = np.random.default_rng(1220)
    first, n_of = _spans(rng.integers(2, 40, 40))
    n = int(n_of.sum())
    costs, gaps = _rows(rng, n), rng.integers(0, 255, (n, 2)).astype(np.uint8)
    got, chars, src, wor = check(f, costs, gaps, first, n_of, rng.integers(0, 6, (66, 66)).astype(np.uint8), 20, 30)
    n_gaps, n_breaks = int((n_of - 1).sum()), sum(g[2] for g in got)
    assert 0.2 * n_gaps <= n_breaks <= 0.8 * n_gaps, (n_breaks, n_gaps)
    got, chars, src, wor = check(f, costs, gaps, first, n_of, rng.integers(0, 256, (66, 66)).astype(np.uint8), 20, 30)
    n_empty = sum(g[2] + 1 - len(set(wor[a:a + m][wor[a:a + m] >= 0].tolist())) for g, a, m in zip(got, first, n_of))
    assert n_empty >= 1, n_empty


def test_two_calls_give_the_same_bytes(S, f):
    rng = np.random.default_rng(1230)
    first, n_of = _spans([70, 0, 200, 5])
    n = int(n_of.sum())
    costs, gaps, B = _rows(rng, n), _gaps(rng, n), rng.integers(0, 40, (66, 66)).astype(np.uint8)
    f.set_bigram(B)
    f.set_word_decode(30, 30)
    a = f.decode_lines(costs, gaps, first, n_of)
    b = f.decode_lines(costs, gaps, first, n_of)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    host = S.decode_lines_host(costs, gaps, first, n_of, B, 30, 30)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, host))
    assert f.line_decode_stats()["table_bytes"] >= 68 * 2 * n


def test_errors_leave_the_context_usable(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    try:
        costs, gaps = np.zeros((3, 65), np.uint8), np.zeros((3, 2), np.uint8)
        with pytest.raises(S.StrErError) as e:                           # no table
            ctx.decode_lines(costs, gaps, [0], [3])
        assert e.value.code == -6 and "bigram" in str(e.value)
        ctx.set_bigram(np.zeros((66, 66), np.uint8))
        ok = ctx.decode_lines(costs, gaps, [0, 3], [3, 0])
        assert LD.as_tuples(ok[0]) == [(0, 3, 0, 3, 0, 0), (0, 0, 0, 0, 0, 0)]
        for first, n_of in (([1], [3]), ([0], [-1]), ([-1], [1]), ([0, 2], [3, 1]), ([2, 0], [1, 2])):
            with pytest.raises(S.StrErError) as e:                       # a window outside the rows, over another or out of order
                ctx.decode_lines(costs, gaps, first, n_of)
            assert e.value.code == -1
        bad = gaps.copy()
        bad[1] = 255
        with pytest.raises(S.StrErError) as e:                           # both moves off at a gap
            ctx.decode_lines(costs, bad, [0], [3])
        assert e.value.code == -1 and "both moves off" in str(e.value)
        bad[1], bad[0] = 0, 255                                          # (the pair of a line's first row is ignored)
        assert ctx.decode_lines(costs, bad, [0, 3], [3, 0])[0].tobytes() == ok[0].tobytes()
        for w in (-1, 128):
            with pytest.raises(S.StrErError) as e:
                ctx.set_line_decode(True, w)
            assert e.value.code == -1
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ctx.decode_lines(costs, gaps, [0, 3], [3, 0]), ok))
    finally:
        ctx.close()
