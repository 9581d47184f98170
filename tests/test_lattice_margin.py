"""The lattice decoder's margins on the GPU (str_er_lattice_margins; the contract is at str_er_lattice_margin): every field of every record,
every per-part array, the edge minima and the full table of marginals against the numpy reference (lattice_margin_ref.py) with ==, at the
kernel's own edges -- words of 0, 1, 31, 32 and 33 atoms made from runs of 0 .. 3 cuts, eight runs of three cuts (32 nodes and 80
edges, the most there are), the words of a workgroup (a wave each), the states 64 and 65 that live past the wave's 64 lanes, the drop
entry, the largest values the 16-bit copies of the forward pass must hold, decoded paths that take pieces and paths that take whole cut
runs."""
import os
import re

import numpy as np
import pytest

import lattice_decode_ref as LD
import lattice_margin_ref as LM
from test_lattice_decode_abi import cheapen, make_rows
from test_word_decode_ref import PAIRS, insertion_vector

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LM_WORDS = 4                      # words of a workgroup of k_lattice_margin (LM_WORDS)
NAMES = ("read_margin", "cut_margin", "read", "alt", "cut_alt", "edge_min", "marginals")


@pytest.fixture(scope="module")
def f(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    yield ctx
    ctx.close()


def _spans(n_of):
    n_of = np.asarray(n_of, np.int64)
    return np.concatenate([[0], np.cumsum(n_of)])[:len(n_of)].astype(np.int32), n_of.astype(np.int32)


def check(S, f, sp, rc, pc, first, n_of, B, ins=0, dele=0, split=8):
    """set_bigram, set_word_decode, set_run_split and lattice_margins against the reference, with and without the tables; returns the
    records as tuples (MARGIN_FIELDS) and the seven arrays in the order of NAMES."""
    f.set_bigram(B)
    f.set_word_decode(ins, dele)
    f.set_run_split(1, 4, split)
    out = f.lattice_margins(sp, rc, pc, first, n_of, want_edges=True, want_marginals=True)
    want = LM.lattice_margins(sp, rc, pc, first, n_of, B, ins, dele, split)
    got = LM.as_tuples(out[0])
    assert out[0].dtype == S.LATTICE_MARGIN_DTYPE and got == want[0], [(w, g, x) for w, (g, x) in enumerate(zip(got, want[0])) if g != x][:5]
    for name, g, x in zip(NAMES, out[1:], want[1:]):
        assert g.dtype == x.dtype and g.shape == x.shape and (g == x).all(), (name, np.argwhere(g != x)[:5])
    bare = f.lattice_margins(sp, rc, pc, first, n_of)
    assert bare[6] is None and bare[7] is None and all(a.tobytes() == b.tobytes() for a, b in zip(bare[:6], out[:6]))
    edges = f.lattice_margins(sp, rc, pc, first, n_of, want_edges=True)
    assert edges[7] is None and edges[6].tobytes() == out[6].tobytes() and edges[0].tobytes() == out[0].tobytes()
    return (got,) + tuple(out[1:])


def test_the_layout_constants_are_the_header_s():
    with open(os.path.join(ROOT, "scene-text-recognition_amd", "csrc", "lattice_margin_kernels.h")) as h:
        txt = h.read()
    for name, v in (("LM_WORDS", LM_WORDS), ("LM_PARTS", 32), ("LM_FROM", 4), ("LM_READINGS", 66)):
        assert int(re.search(r"constexpr int " + name + r" = (\d+);", txt).group(1)) == v


# 0, 1, 31, 32 and 33 atoms from runs of 0 .. 3 cuts; eight runs of three cuts: 32 nodes and 80 edges
WORDS = [[], [0], [1], [2], [3], [0, 3, 0], [3] * 7 + [2], [3] * 7 + [1, 0], [3] * 8, [0] * 32, [1] * 16, [3] * 8 + [0], [0] * 33, [2] * 11, [3, 3, 2, 1, 0]]
ATOMS = [sum(k + 1 for k in w) for w in WORDS]


@pytest.mark.parametrize("ins,dele", PAIRS)
def test_every_shape_of_word_under_every_pair_of_moves(S, f, ins, dele):
    assert ATOMS[:5] == [0, 1, 2, 3, 4] and ATOMS[6:14] == [31, 31, 32, 32, 32, 33, 33, 33]
    rng = np.random.default_rng(3000 + ins + 7 * dele)
    first, n_of = _spans([len(w) for w in WORDS])
    sp, rc, pc = make_rows(S, rng, np.array([k for w in WORDS for k in w]))
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    B = rng.integers(0, 256, (66, 66)).astype(np.uint8)
    split = (8, 0, 255)[(ins + dele) % 3]
    got, rm, cm, rd, al, ca, em, mg = check(S, f, sp, rc, pc, first, n_of, B, ins, dele, split)
    for w, N in enumerate(ATOMS):
        if N == 0 or N > 32:                                        # no atoms, and not decoded
            assert got[w] == LM.NONE_RECORD and (rm[w] == -1).all() and (cm[w] == -1).all() and (rd[w] == 255).all() and (al[w] == 255).all() and (ca[w] == 255).all()
            assert (em[w] == -1).all() and (mg[w] == -1).all()
            continue
        n_edges = sum((k + 1) * (k + 2) // 2 for k in WORDS[w])
        p = int((rm[w] >= 0).sum())
        assert got[w][7] == n_edges == (em[w] >= 0).sum() and len(WORDS[w]) <= p <= N and got[w][0] == rm[w, :p].min() >= 0 and (rm[w, p:] == -1).all()
        assert (mg[w][em[w] >= 0][:, :65] >= 0).all() and ((mg[w][em[w] >= 0][:, 65] >= 0) == (dele > 0)).all() and (mg[w][em[w] < 0] == -1).all()
        assert (got[w][4] >= 0) == (max(WORDS[w]) > 0) and (rd[w, :p] <= 65).all() and (rd[w, p:] == 255).all()
    assert got[8][7] == 80
    # a cheap table beside dear runs and cheap pieces, so that the moves and the cuts are taken where they are on: the drop entry is read
    # and is the alternative, the decoded paths take pieces
    B2 = rng.integers(0, 6, (66, 66)).astype(np.uint8)
    rc2, pc2 = (150 + rc // 4).astype(np.uint8), (pc // 4).astype(np.uint8)
    rc2[::3] = 250                                                  # (and rows that say nothing: dropping them is cheaper than any reading)
    pc2[::5] = 250
    rc2[1::3, 5] = 0                                                # (and rows with one reading: the next best thing is to drop them)
    got, rm, cm, rd, al, ca, em, mg = check(S, f, sp, rc2, pc2, first, n_of, B2, ins, dele, split)
    if 0 < dele < 255:
        assert (rd == 65).any() and (dele == 1 or (al == 65).any())          # (DEL = 1 drops every part: the drop is never the alternative)
    if split < 255:
        assert any((rm[w] >= 0).sum() > len(WORDS[w]) for w in range(len(WORDS)) if 0 < ATOMS[w] <= 32)


def test_word_counts_around_a_workgroup(S, f):
    rng = np.random.default_rng(32)
    B = rng.integers(0, 64, (66, 66)).astype(np.uint8)
    for n in (0, 1, LM_WORDS - 1, LM_WORDS, LM_WORDS + 1, 257):
        first, n_of = _spans(rng.integers(0, 4 if n == 257 else 7, n))
        sp, rc, pc = make_rows(S, rng, rng.integers(0, 4, int(n_of.sum())))
        out = check(S, f, sp, cheapen(rng, rc), cheapen(rng, pc), first, n_of, B, 20, 30, 8)
        assert len(out[0]) == n and out[1].shape == (n, 32) and out[3].shape == (n, 32) and out[6].shape == (n, 32, 4) and out[7].shape == (n, 32, 4, 66)
    none = f.lattice_margins(np.zeros(0, S.RUN_SPLIT_DTYPE), np.zeros((0, 65), np.uint8), np.zeros((0, 65), np.uint8), [], [], want_edges=True, want_marginals=True)
    assert none[0].shape == (0,) and none[0].dtype == S.LATTICE_MARGIN_DTYPE and none[7].shape == (0, 32, 4, 66)


def test_paths_that_take_pieces_and_paths_that_take_whole_cut_runs(S, f):
    rng = np.random.default_rng(33)
    cuts = [3, 1, 2, 0, 3]
    first, n_of = _spans([len(cuts)])
    sp, rc, pc = make_rows(S, rng, np.array(cuts))
    B = rng.integers(0, 8, (66, 66)).astype(np.uint8)
    taken = []
    for rows_r, rows_p in (((150 + rc // 4).astype(np.uint8), pc // 8), (rc // 8, (150 + pc // 4).astype(np.uint8))):
        for ins, dele in ((0, 0), (20, 30)):
            got, rm, cm, rd, al, ca, em, mg = check(S, f, sp, rows_r, rows_p, first, n_of, B, ins, dele, 8)
            p = int((rm[0] >= 0).sum())
            taken.append(p)
            assert got[0][4] >= 0 and (cm[0, :p] >= 0).sum() >= p - 1 and got[0][7] == 10 + 3 + 6 + 1 + 10
    assert taken[0] > len(cuts) and taken[1] > len(cuts) and taken[2] == taken[3] == len(cuts)          # pieces, and whole cut runs


def test_constant_inputs(S, f):
    rng = np.random.default_rng(34)
    zero_t, full_t = np.zeros((66, 66), np.uint8), np.full((66, 66), 255, np.uint8)
    for cuts in ([0], [3], [1, 2], [3] * 8):
        first, n_of = _spans([len(cuts)])
        sp, rc, pc = make_rows(S, rng, np.array(cuts))
        R = len(cuts)
        for ins, dele in PAIRS:                                     # all zero: every margin is 0, the reading 0, the alternative 1, the whole runs the path
            got, rm, cm, rd, al, ca, em, mg = check(S, f, sp, rc * 0, pc * 0, first, n_of, zero_t, ins, dele, 0)
            assert got[0][:4] == (0, 0, 0, 1) and (rm[0, :R] == 0).all() and (rd[0, :R] == 0).all() and (al[0, :R] == 1).all() and (rm[0, R:] == -1).all()
            if max(cuts):
                k = [c > 0 for c in cuts].index(True)
                assert got[0][4:7] == (0, k, 0 | 1 << 4)
        check(S, f, sp, rc * 0, pc * 0, first, n_of, zero_t, 64, 64, 8)
    # all 255 at 32 nodes -- rows, table, SPLIT, INS and DEL: the largest values the narrow copies in LDS must hold
    cuts = [3] * 8
    first, n_of = _spans([8])
    sp, rc, pc = make_rows(S, rng, np.array(cuts))
    rc[:] = 255
    pc[:] = 255
    got, rm, cm, rd, al, ca, em, mg = check(S, f, sp, rc, pc, first, n_of, full_t, 0, 0, 255)
    assert got[0] == (0, 0, 0, 1, 3 * 255, 0, 0 | 1 << 4, 80) and int(mg.max()) == (8 + 7 * 2 + 1) * 255 and (mg[0, :, :, 65] == -1).all()
    got, rm, cm, rd, al, ca, em, mg = check(S, f, sp, rc, pc, first, n_of, full_t, 255, 255, 255)
    assert got[0][:4] == (255, 0, 65, 0) and (rd[0, :8] == 65).all() and int(mg.max()) <= 41055
    # the dearest path there is: every atom its own part, read, with a character inserted behind it
    for r in range(8):
        for i in range(4):
            pc[int(sp["first_piece"][r]) + LD.piece_of(4, i, i + 1)] = 254
    got, rm, cm, rd, al, ca, em, mg = check(S, f, sp, rc, pc, first, n_of, full_t, 255, 0, 255)
    assert int(mg.max()) <= 41055
    check(S, f, sp, rc, pc, first, n_of, zero_t, 255, 255, 255)
    check(S, f, sp, rc * 0, pc * 0, first, n_of, full_t, 255, 255, 255)


def test_paths_through_the_states_past_the_wave(S, f):
    """The vectors of test_word_margin.py on a lattice: readings and alternatives among 63, 64 and 65 through runs and pieces."""
    rng = np.random.default_rng(35)
    cuts = [1, 0, 2]
    sp, rc, pc = make_rows(S, rng, np.array(cuts))
    rc[:] = 60
    pc[:] = 9
    B = np.full((66, 66), 200, np.uint8)
    B[65, 64] = B[64, 63] = B[63, 64] = 1
    B[63, 65] = 2
    got, rm, cm, rd, al, ca, em, mg = check(S, f, sp, rc, pc, [0], [3], B, 0, 0, 0)          # ")(" over the parts
    p = int((rm[0] >= 0).sum())
    assert rd[0, :p].tolist() == ([64, 63] * 3)[:p] and (rm[0, :p] > 0).all()
    pc2 = pc.copy()
    pc2[1, :] = 250
    got, rm, cm, rd, al, ca, em, mg = check(S, f, sp, rc, pc2, [0], [3], B, 3, 4, 8)
    p = int((rm[0] >= 0).sum())
    assert set(rd[0, :p].tolist()) <= {63, 64, 65} and set(al[0, :p].tolist()) & {63, 64, 65}
    # label 64 against label 0 on a zero table: a tie, the reading 0 and the alternative 64; then 64 alone cheaper, and 0 the alternative
    tie_r, tie_p = np.full((3, 65), 100, np.uint8), np.full((len(pc), 65), 100, np.uint8)
    tie_r[:, 0] = tie_r[:, 64] = 7
    got, rm, cm, rd, al, ca, em, mg = check(S, f, sp, tie_r, tie_p, [0], [3], np.zeros((66, 66), np.uint8))
    assert got[0][:4] == (0, 0, 0, 64) and al[0, :3].tolist() == [64] * 3
    tie_r[:, 64] = 6
    got, rm, cm, rd, al, ca, em, mg = check(S, f, sp, tie_r, tie_p, [0], [3], np.zeros((66, 66), np.uint8))
    assert got[0][:4] == (1, 0, 64, 0) and rd[0, :3].tolist() == [64] * 3
    tie_p[:, 64] = 1                                                # ... and through the pieces
    got, rm, cm, rd, al, ca, em, mg = check(S, f, sp, tie_r, tie_p, [0], [3], np.zeros((66, 66), np.uint8), 0, 0, 0)
    assert rd[0, :5].tolist() == [64] * 5 and rd[0, 5] == 255
    # INS of 64 behind 63 and of 63 behind 64 on random rows with those two cheap, the words overlapping
    first, n_of = _spans([6, 3, 1, 5])
    first[1:] = [0, 5, 2]
    sp, rc, pc = make_rows(S, rng, rng.integers(0, 4, 7))
    rc, pc = (100 + rc // 2).astype(np.uint8), (100 + pc // 2).astype(np.uint8)
    rc[:, 63:] = rng.integers(0, 4, (len(rc), 2))
    pc[:, 63:] = rng.integers(0, 4, (len(pc), 2))
    B = rng.integers(100, 256, (66, 66)).astype(np.uint8)
    B[63, 64] = B[64, 63] = B[65, 63] = B[65, 64] = B[63, 65] = B[64, 65] = 0
    got, rm, cm, rd, al, ca, em, mg = check(S, f, sp, rc, pc, first, n_of, B, 2, 2, 1)
    p = int((rm[0] >= 0).sum())
    assert set(rd[0, :p].tolist()) <= {63, 64, 65}
    # the 64-character vector: an insertion after every run, the inserted characters have no part
    C, B = insertion_vector()
    sp, rc, pc = make_rows(S, rng, np.zeros(32, np.int64))
    got, rm, cm, rd, al, ca, em, mg = check(S, f, sp, C, pc, [0], [32], B, 1, 0, 8)
    assert (rd[0] == 63).all() and got[0][0] > 0 and got[0][4:] == (-1, -1, -1, 32) and (mg[0, np.arange(32), 0, 63] == 32).all()


def test_uncut_words_equal_the_word_margins_on_the_same_rows(S, f):
    rng = np.random.default_rng(36)
    first, n_of = _spans([5, 1, 32, 0, 17, 33, 2])
    sp, rc, pc = make_rows(S, rng, np.zeros(int(n_of.sum()), np.int64))
    rc = cheapen(rng, rc)
    for ins, dele in PAIRS[:4]:
        B = rng.integers(0, 256 if ins else 32, (66, 66)).astype(np.uint8)
        got, rm, cm, rd, al, ca, em, mg = check(S, f, sp, rc, pc, first, n_of, B, ins, dele, 8)
        rec, wm, wr, wa, wg = f.word_margins(rc, first, n_of, want_marginals=True)
        assert rm.tobytes() == wm.tobytes() and rd.tobytes() == wr.tobytes() and al.tobytes() == wa.tobytes()
        assert [g[:4] for g in got] == [tuple(int(r[k]) for k in rec.dtype.names) for r in rec]
        assert (cm == -1).all() and (ca == 255).all() and all(g[4:7] == (-1, -1, -1) for g in got) and (mg[:, :, 0] == wg).all() and (mg[:, :, 1:] == -1).all()


def test_overlapping_words_and_a_repeat_call(S, f):
    rng = np.random.default_rng(37)
    sp, rc, pc = make_rows(S, rng, rng.integers(0, 4, 9))
    rc, pc = (120 + cheapen(rng, rc) // 2).astype(np.uint8), (cheapen(rng, pc) // 3).astype(np.uint8)
    B = rng.integers(0, 40, (66, 66)).astype(np.uint8)
    out = check(S, f, sp, rc, pc, [0, 0, 3, 2], [9, 9, 6, 4], B, 30, 30, 8)
    assert out[0][0] == out[0][1] and out[7][0].tobytes() == out[7][1].tobytes() and out[1][0].tobytes() == out[1][1].tobytes()
    again = f.lattice_margins(sp, rc, pc, [0, 0, 3, 2], [9, 9, 6, 4], want_edges=True, want_marginals=True)
    assert LM.as_tuples(again[0]) == out[0] and all(a.tobytes() == b.tobytes() for a, b in zip(again[1:], out[1:]))
    host = S.lattice_margins_host(sp, rc, pc, [0, 0, 3, 2], [9, 9, 6, 4], B, 30, 30, 8, want_edges=True, want_marginals=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(host, again))
    # the decoder's own call is not disturbed: its buffer is its own
    before = f.lattice_decode_stats()
    f.lattice_margins(sp, rc, pc, [0], [9])
    assert f.lattice_decode_stats() == before


def test_errors_leave_the_context_usable(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    try:
        rng = np.random.default_rng(38)
        sp, rc, pc = make_rows(S, rng, np.array([1, 0]))
        with pytest.raises(S.StrErError) as e:                           # no table
            ctx.lattice_margins(sp, rc, pc, [0], [2])
        assert e.value.code == -6 and "bigram" in str(e.value)
        ctx.set_bigram(np.zeros((66, 66), np.uint8))
        out = ctx.lattice_margins(sp, rc, pc, [0, 0], [2, 0])
        assert LM.as_tuples(out[0])[1] == LM.NONE_RECORD and LM.as_tuples(out[0])[0][7] == 4
        for first, n_of in (([1], [2]), ([0], [-1]), ([-1], [1])):
            with pytest.raises(S.StrErError) as e:                       # a word outside the runs
                ctx.lattice_margins(sp, rc, pc, first, n_of)
            assert e.value.code == -1
        bad = sp.copy()
        bad["n_cuts"][0] = 4
        with pytest.raises(S.StrErError) as e:
            ctx.lattice_margins(bad, rc, pc, [0], [2])
        assert e.value.code == -1
        assert ctx.lattice_decode_stats() == 0                           # (the decoder's buffer was never made)
        again = ctx.lattice_margins(sp, rc, pc, [0, 0], [2, 0])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:6], out[:6]))
    finally:
        ctx.close()
