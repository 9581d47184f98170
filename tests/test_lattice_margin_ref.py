"""The numpy reference of the lattice decoder's margins (lattice_margin_ref.py, written from the definition at str_er_lattice_margin): its
backward form against an enumeration of every path that keeps the minimum per (edge, reading) on alphabets of 2 and 3 labels and
lattices of up to 5 atoms under the four move settings; the atom-cover identity; cut_margin against the cheapest path with another part
sequence; the uncut case against word_margin_ref at 65 labels; and the host entry point (str_er_lattice_margins_host) against the
reference with == on every output.  No GPU."""
import numpy as np
import pytest

import lattice_decode_ref as LD
import lattice_margin_ref as LM
import word_margin_ref as WG
from test_lattice_decode_abi import cheapen, make_rows
from test_lattice_decode_ref import random_word

MOVES = ((0, 0), (5, 0), (0, 7), (3, 4))          # off, each move alone, both
# cut counts per run: up to 3 atoms at 3 labels, up to 5 atoms at 2 labels (the enumeration grows with moves ^ edges)
SHAPES = {3: [(0,), (1,), (2,), (0, 0), (0, 1), (1, 0)], 2: [(3,), (1, 1), (2, 0), (0, 2), (1, 2), (3, 0), (0, 1, 0), (0, 0, 2)]}


def words(n):
    """(cuts, first pieces, run rows, piece rows, table, SPLIT) of the enumerated cases at n labels, the same for every move setting."""
    rng = np.random.default_rng(400 + n)
    for cuts in SHAPES[n]:
        for rep in range(3 if n == 3 else 1 if sum(k + 1 for k in cuts) == 5 else 2):
            hi = (4, 16, 256)[(rep + len(cuts)) % 3]                  # small ranges tie often
            split = (0, 8, 255)[(rep + sum(cuts)) % 3]
            fp, runs, pieces = random_word(rng, cuts, n, hi)
            yield cuts, fp, runs, pieces, rng.integers(0, hi, (n + 1, n + 1)), split


@pytest.mark.parametrize("ins,dele", MOVES)
@pytest.mark.parametrize("n", (2, 3))
def test_reference_equals_the_enumeration_of_every_path(n, ins, dele):
    cases = cut_words = 0
    for cuts, fp, runs, pieces, B, split in words(n):
        L = LD.Word(cuts, fp, runs, pieces, 0, n)
        cost, M = LM.edge_marginals(L, B, ins, dele, split, n)
        best, EM, S = LM.enumerate_paths(L, B, ins, dele, split, n)
        assert cost == best == LD.enumerate_best(cuts, fp, runs, pieces, B, ins, dele, split, n)
        assert set(M) == set(EM) and len(M) == sum((k + 1) * (k + 2) // 2 for k in cuts)
        for e in M:                                                   # every edge marginal
            assert (M[e] == EM[e]).all(), (cuts, ins, dele, split, e, M[e], EM[e])
            assert ((M[e][:n] >= 0).all()) and (M[e][n] >= 0) == (dele > 0)
        # the atom-cover identity: every path covers every atom with exactly one edge
        for r, A in enumerate(L.atoms):
            for t in range(A):
                assert min(LM.edge_min(M[r, i, j]) for (q, i, j) in M if q == r and i <= t < j) == cost
        # the margins of the decoded path
        R = LM.margins_word(cuts, fp, runs, pieces, B, ins, dele, split, 0, n)
        assert R["cost"] == cost and S[tuple(R["edges"])] == cost
        others = [v for seq, v in S.items() if seq != tuple(R["edges"])]
        if others:                                                    # cut_margin: the cheapest path with another part sequence
            assert R["rec"][4] + cost == min(others) and R["rec"][4] >= 0
            k = R["rec"][5]
            i, j = R["rec"][6] & 15, R["rec"][6] >> 4
            r = R["edges"][k][0]
            assert (r, i, j) not in R["edges"] and LM.edge_min(M[r, i, j]) == cost + R["rec"][4] and R["cut_margin"][k] == R["rec"][4]
            cut_words += 1
        else:
            assert R["rec"][4:7] == (-1, -1, -1) and max(cuts) == 0
        for k, (r, i, j) in enumerate(R["edges"]):
            assert (R["cut_margin"][k] == -1) == (R["cut_alt"][k] == 0xFF) == (cuts[r] == 0)
            assert R["read_margin"][k] >= 0 and R["alt"][k] != R["read"][k] and M[r, i, j][R["alt"][k]] == cost + R["read_margin"][k]
        assert R["rec"][7] == len(M) and R["rec"][0] == min(R["read_margin"])
        cases += 1
    assert cases == (18 if n == 3 else 13) and cut_words > cases // 2


@pytest.mark.parametrize("ins,dele", MOVES)
def test_uncut_words_equal_the_word_margins_at_65_labels(ins, dele):
    rng = np.random.default_rng(500 + ins + dele)
    for m in (1, 2, 9, 32):
        rows = np.where(rng.random((m, 65)) < 0.1, rng.integers(0, 24, (m, 65)), rng.integers(60, 256, (m, 65)))
        B = rng.integers(0, 6 if m % 2 else 256, (66, 66))
        R = LM.margins_word([0] * m, [0] * m, rows, np.zeros((0, 65)), B, ins, dele, 8)
        rec, row_margin, read, alt, M, cost = WG.margins_word(rows, B, ins, dele)
        assert R["rec"] == rec + (-1, -1, -1, m) and R["cost"] == cost
        assert R["read_margin"] == row_margin and R["read"] == read and R["alt"] == alt
        assert R["cut_margin"] == [-1] * m and R["cut_alt"] == [0xFF] * m
        for r in range(m):
            assert (R["M"][r, 0, 1] == M[r]).all()
    for m in (0, 33):
        assert LM.margins_word([0] * m, [0] * m, np.zeros((m, 65)), np.zeros((0, 65)), np.zeros((66, 66)))["rec"] == LM.NONE_RECORD


def same(S, got, want):
    rec, rm, cm, rd, al, ca, em, mg = got
    assert rec.dtype == S.LATTICE_MARGIN_DTYPE and LM.as_tuples(rec) == want[0], [(w, g, x) for w, (g, x) in enumerate(zip(LM.as_tuples(rec), want[0])) if g != x][:5]
    for name, g, x in zip(("read_margin", "cut_margin", "read", "alt", "cut_alt", "edge_min", "marginals"), (rm, cm, rd, al, ca, em, mg), want[1:]):
        assert g.dtype == x.dtype and g.shape == x.shape and (g == x).all(), (name, np.argwhere(g != x)[:5])


def test_the_host_entry_point_equals_the_reference(S):
    rng = np.random.default_rng(31)
    shapes = [[], [0], [1], [2], [3], [0, 3, 0], [3] * 8, [0] * 32, [3] * 8 + [0], [0] * 33, [3, 3, 2, 1, 0]] + [list(rng.integers(0, 4, int(k))) for k in rng.integers(1, 9, 12)]
    n_of = np.array([len(w) for w in shapes])
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]])
    sp, rc, pc = make_rows(S, rng, np.array([k for w in shapes for k in w]))
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    for (ins, dele), split in zip(MOVES + ((255, 255),), (8, 0, 255, 8, 255)):
        B = rng.integers(0, 256, (66, 66)).astype(np.uint8) if ins != 3 else rng.integers(0, 3, (66, 66)).astype(np.uint8)
        want = LM.lattice_margins(sp, rc, pc, first, n_of, B, ins, dele, split)
        got = S.lattice_margins_host(sp, rc, pc, first, n_of, B, ins, dele, split, want_edges=True, want_marginals=True)
        same(S, got, want)
        for w in (0, 8, 9):                                           # no runs; N = 33 twice: not decoded
            assert want[0][w] == LM.NONE_RECORD and (got[1][w] == -1).all() and (got[3][w] == 255).all() and (got[6][w] == -1).all() and (got[7][w] == -1).all()
        assert want[0][6][7] == 80 and want[0][7][7] == 32 and (got[6][6] >= 0).sum() == 80
        bare = S.lattice_margins_host(sp, rc, pc, first, n_of, B, ins, dele, split)
        assert bare[6] is None and bare[7] is None and all(a.tobytes() == b.tobytes() for a, b in zip(bare[:6], got[:6]))
    # cheap pieces under dear runs, so that the decoded paths take pieces; dear pieces, so that they take whole cut runs
    B = rng.integers(0, 8, (66, 66)).astype(np.uint8)
    for rows_r, rows_p, pieces_taken in (((150 + rc // 4).astype(np.uint8), pc // 8, True), (rc // 8, (150 + pc // 4).astype(np.uint8), False)):
        want = LM.lattice_margins(sp, rows_r, rows_p, first, n_of, B, 20, 30, 8)
        same(S, S.lattice_margins_host(sp, rows_r, rows_p, first, n_of, B, 20, 30, 8, want_edges=True, want_marginals=True), want)
        n_parts = [(want[1][w] >= 0).sum() for w in range(len(shapes))]
        assert pieces_taken == any(n_parts[w] > n_of[w] for w in range(len(shapes)))
        assert any(r[4] >= 0 for r in want[0])
    # the checks of the decoder's host entry point
    for bad in (([1], [len(rc)]), ([0], [-1]), ([-1], [1])):
        with pytest.raises(S.StrErError) as e:
            S.lattice_margins_host(sp, rc, pc, *bad, B)
        assert e.value.code == -1
    with pytest.raises(S.StrErError):
        S.lattice_margins_host(sp, rc, pc, [0], [1], B, 256, 0)
    with pytest.raises(S.StrErError):
        S.lattice_margins_host(sp, rc, pc, [0], [1], B, 0, 0, 256)
    out = S.lattice_margins_host(sp, rc, pc, [], [], B, want_edges=True, want_marginals=True)
    assert out[0].shape == (0,) and out[1].shape == (0, 32) and out[5].shape == (0, 32) and out[6].shape == (0, 32, 4) and out[7].shape == (0, 32, 4, 66)
