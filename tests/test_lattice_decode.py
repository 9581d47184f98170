"""The joint decode over the piece lattice on the GPU (str_er_lattice_decode_words; the contract is at str_er_lattice_decode): every
field of every record, every byte of the strings and every part against the host entry point and the numpy reference
(lattice_decode_ref.py) with ==, at the kernel's own edges -- words without runs, runs of 1 .. 4 atoms, N = 32 and 33, the words of a
workgroup (a wave each) and a full pass, a cut run between uncut ones (the ring of products is per run), the tie rules on constant
inputs, the states 64 and 65 that live past the wave's 64 lanes, everything at 255 for the keys' bits, and the uncut words against the
word decoder on the same rows."""
import numpy as np
import pytest

import lattice_decode_ref as LD
import word_decode_ref as WD
from test_lattice_decode_abi import MOVES, cheapen, make_rows

pytestmark = pytest.mark.gpu
WG_WORDS = 4                      # words of a workgroup of k_lattice_decode (LD_WORDS)


@pytest.fixture(scope="module")
def f(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    yield ctx
    ctx.close()


def _spans(n_of):
    n_of = np.asarray(n_of, np.int64)
    return np.concatenate([[0], np.cumsum(n_of)])[:len(n_of)].astype(np.int32), n_of.astype(np.int32)


def check(S, f, sp, rc, pc, first, n_of, B, ins=0, dele=0, split=8):
    """set_bigram, set_word_decode, set_run_split and lattice_decode_words against the host entry point and the reference; returns the
    records as tuples (LATTICE_FIELDS), chars, src and the parts as (run, piece) rows."""
    f.set_bigram(B)
    f.set_word_decode(ins, dele)
    f.set_run_split(1, 4, split)
    dec, chars, src, parts = f.lattice_decode_words(sp, rc, pc, first, n_of)
    assert dec.dtype == S.LATTICE_DECODE_DTYPE and parts.dtype == S.SPLIT_PART_DTYPE and chars.shape == src.shape == (len(first), 64)
    hd, hc, hs, hp = S.lattice_decode_words_host(sp, rc, pc, first, n_of, B, ins, dele, split)
    assert dec.tobytes() == hd.tobytes() and chars.tobytes() == hc.tobytes() and src.tobytes() == hs.tobytes() and parts.tobytes() == hp.tobytes(), \
        [w for w in range(len(dec)) if dec[w] != hd[w] or (chars[w] != hc[w]).any() or (src[w] != hs[w]).any()][:5]
    want = LD.decode_words(sp, rc, pc, first, n_of, B, ins, dele, split)
    got = LD.as_tuples(dec)
    assert got == want[0], [(w, g, x) for w, (g, x) in enumerate(zip(got, want[0])) if g != x][:5]
    assert (chars == want[1]).all() and (src == want[2]).all(), np.argwhere((chars != want[1]) | (src != want[2]))[:5]
    pr = np.stack([parts["run"], parts["piece"]], 1)
    assert pr.tolist() == want[3].tolist()
    return got, chars, src, pr


@pytest.mark.parametrize("ins,dele,split", MOVES)
def test_every_shape_of_word_under_every_set_of_moves(S, f, ins, dele, split):
    """No runs; one uncut run; one run with 1, 2 and 3 cuts; a cut run between two uncut ones; N = 32 as 8 runs of 4 atoms and as 32
    uncut runs; N = 33, which is not decoded and whose read_cost is still made."""
    rng = np.random.default_rng(2000 + ins + 7 * dele + split)
    words = [[], [0], [1], [2], [3], [0, 3, 0], [0, 1, 0, 2], [3] * 8, [0] * 32, [3] * 8 + [0], [0] * 33, [3, 3, 2, 1, 0]]
    first, n_of = _spans([len(w) for w in words])
    sp, rc, pc = make_rows(S, rng, np.array([k for w in words for k in w]))
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    B = rng.integers(0, 256, (66, 66)).astype(np.uint8)
    got, chars, src, parts = check(S, f, sp, rc, pc, first, n_of, B, ins, dele, split)
    assert got[0] == (int(B[65, 65]), int(B[65, 65]), 0, 0, 0, 0, 0, 0)
    for w in (9, 10):
        assert got[w][0] == -1 and got[w][2:6] == (0, 0, 0, 0) and got[w][7] == 0 and (chars[w] == 255).all() and (src[w] == 255).all()
        assert got[w][1] == WD.read_cost(rc[first[w]:first[w] + n_of[w]], B)
    for w, g in enumerate(got):
        if g[0] >= 0:
            N = sum(k + 1 for k in words[w])
            assert g[0] <= g[1] and g[3] + g[5] == g[2] and g[3] + g[4] == g[7] and len(words[w]) <= g[7] <= N <= 32
    assert [g[6] for g in got] == np.concatenate([[0], np.cumsum([g[7] for g in got])])[:-1].tolist()
    # a table of cheap and dear pairs beside dear runs and cheap pieces, so that the moves and the cuts are taken where they are on
    B2 = np.where(rng.random((66, 66)) < 0.5, rng.integers(0, 6, (66, 66)), 200).astype(np.uint8)
    rc2, pc2 = (150 + rc // 4).astype(np.uint8), (120 + pc // 4).astype(np.uint8)          # (one cheap label a row: the string is the rows', the table has to be bridged)
    rc2[np.arange(len(rc2)), rng.integers(0, 65, len(rc2))] = 60
    pc2[np.arange(len(pc2)), rng.integers(0, 65, len(pc2))] = 0
    got, _, _, parts = check(S, f, sp, rc2, pc2, first, n_of, B2, ins, dele, split)
    if 0 < ins < 255:
        assert sum(g[5] for g in got) > 0
    if 0 < dele < 255:
        assert sum(g[4] for g in got) > 0
    if split < 255:
        assert (parts[:, 1] >= 0).any()


def test_word_counts_around_a_workgroup_and_a_full_pass(S, f):
    rng = np.random.default_rng(2)
    B = rng.integers(0, 64, (66, 66)).astype(np.uint8)
    for n in (0, 1, WG_WORDS, WG_WORDS + 1, 1000):
        first, n_of = _spans(rng.integers(0, 5 if n == 1000 else 9, n))
        sp, rc, pc = make_rows(S, rng, rng.integers(0, 4, int(n_of.sum())))
        got, chars, src, parts = check(S, f, sp, cheapen(rng, rc), cheapen(rng, pc), first, n_of, B, 20, 30, 8)
        assert len(got) == n and chars.shape == (n, 64) and src.shape == (n, 64)
    dec, chars, src, parts = f.lattice_decode_words(np.zeros(0, S.RUN_SPLIT_DTYPE), np.zeros((0, 65), np.uint8), np.zeros((0, 65), np.uint8), [], [])
    assert dec.shape == (0,) and dec.dtype == S.LATTICE_DECODE_DTYPE and parts.shape == (0,)


def test_the_ring_of_products_does_not_cross_a_run_boundary(S, f):
    """A run of 4 atoms between two uncut runs, and the same runs the other way round: were a product of the run before still read as a
    local node of this one, the dear rows behind it would show up in the cost.  Every piece row but those on one path is dear."""
    rng = np.random.default_rng(6)
    for cuts in ([0, 3, 0], [3, 0, 3], [2, 3, 1], [0, 0, 3, 3, 0, 0]):
        first, n_of = _spans([len(cuts)])
        sp, rc, pc = make_rows(S, rng, np.array(cuts))
        rc[:] = rng.integers(200, 256, rc.shape)
        pc[:] = rng.integers(200, 256, pc.shape)
        for r, k in enumerate(cuts):                                    # the atoms (i, i + 1) of every cut run read cheap, each its own label
            for i in range(k + 1 if k else 0):
                pc[int(sp["first_piece"][r]) + LD.piece_of(k + 1, i, i + 1), (7 * r + i) % 65] = 1
        B = rng.integers(0, 4, (66, 66)).astype(np.uint8)
        got, chars, src, parts = check(S, f, sp, rc, pc, first, n_of, B, 0, 0, 8)
        assert got[0][7] == sum(k + 1 for k in cuts) and chars[0, :got[0][2]].tolist() == [(7 * r + i) % 65 for r, k in enumerate(cuts) for i in range(k + 1)] or 0 in cuts
        for ins, dele, split in MOVES[1:]:
            check(S, f, sp, rc, pc, first, n_of, B, ins, dele, split)


def test_constant_inputs_where_every_tie_rule_decides(S, f):
    rng = np.random.default_rng(8)
    for cuts in ([0], [3], [1, 2], [3] * 8, [0] * 32):
        first, n_of = _spans([len(cuts)])
        sp, rc, pc = make_rows(S, rng, np.array(cuts))
        R = len(cuts)
        for ins, dele, split in MOVES + ((64, 64, 0),):
            zero_t, full_t = np.zeros((66, 66), np.uint8), np.full((66, 66), 255, np.uint8)
            # all rows and the whole table equal: the smaller i, SUB before DEL and the smaller a decide everything
            got, chars, src, parts = check(S, f, sp, rc * 0, pc * 0, first, n_of, zero_t, ins, dele, split)
            assert got[0] == (0, 0, R, R, 0, 0, 0, R) and (chars[0, :R] == 0).all() and src[0, :R].tolist() == list(range(R)) and (parts[:, 1] == -1).all()
            check(S, f, sp, rc * 0 + 255, pc * 0 + 255, first, n_of, full_t, ins, dele, split)
            check(S, f, sp, rc * 0, pc * 0, first, n_of, full_t, ins, dele, split)
            check(S, f, sp, rc * 0 + 255, pc * 0 + 255, first, n_of, zero_t, ins, dele, split)
    # rows where only the order of i decides: a run of 3 atoms whose whole, (0, 1) + (1, 3), (0, 2) + (2, 3) and atoms all cost 12 at SPLIT = 0
    sp, rc, pc = make_rows(S, rng, np.array([2]))
    rc[:] = 12
    pc[:] = 8
    pc[[LD.piece_of(3, 0, 1), LD.piece_of(3, 1, 2), LD.piece_of(3, 2, 3)]] = 4
    got, chars, src, parts = check(S, f, sp, rc, pc, [0], [1], np.zeros((66, 66), np.uint8), 0, 0, 0)
    assert got[0][0] == 12 and parts.tolist() == [[0, -1]]
    pc[LD.piece_of(3, 0, 1)] = 3                                        # (0, 1) cheaper: into node 3 the edges from 1 and from 2 tie at 11: from 1
    pc[LD.piece_of(3, 0, 2)] = 7
    got, chars, src, parts = check(S, f, sp, rc, pc, [0], [1], np.zeros((66, 66), np.uint8), 0, 0, 0)
    assert got[0][0] == 11 and parts[:, 1].tolist() == [LD.piece_of(3, 0, 1), LD.piece_of(3, 1, 3)]
    # rows where only SUB before DEL decides: the second run reads for what dropping it costs
    sp, rc, pc = make_rows(S, rng, np.array([0, 0]))
    rc[:] = 3
    empty_dear = np.zeros((66, 66), np.uint8)
    empty_dear[65, 65] = 9                                              # (so that dropping both is not the cheapest)
    got, chars, src, parts = check(S, f, sp, rc, pc, [0], [2], empty_dear, 0, 3, 8)
    assert got[0][:6] == (6, 6, 2, 2, 0, 0)
    got, chars, src, parts = check(S, f, sp, rc, pc, [0], [2], empty_dear, 0, 2, 8)
    assert got[0][0] == 5 and got[0][3:5] == (1, 1) and src[0, 0] == 1
    # the same between a piece and a drop of it behind a cut: DEL + SPLIT against row + SPLIT
    sp, rc, pc = make_rows(S, rng, np.array([1]))
    rc[:] = 40
    pc[:] = 3
    empty_dear[65, 65] = 200
    got, chars, src, parts = check(S, f, sp, rc, pc, [0], [1], empty_dear, 0, 3, 8)
    assert got[0][0] == 14 and got[0][3:5] == (2, 0) and got[0][7] == 2


def test_everything_at_255_for_the_keys_bits(S, f):
    """Rows, table, SPLIT, INS and DEL all 255 on the longest words: the largest values the keys carry."""
    full_t = np.full((66, 66), 255, np.uint8)
    rng = np.random.default_rng(9)
    cuts = [3] * 8 + [0] * 32 + [3] * 8 + [0]
    first, n_of = _spans([8, 32, 9])
    sp, rc, pc = make_rows(S, rng, np.array(cuts))
    rc[:] = 255
    pc[:] = 255
    got, chars, src, parts = check(S, f, sp, rc, pc, first, n_of, full_t, 255, 255, 255)
    assert got[0][:6] == (9 * 255, 17 * 255, 0, 0, 8, 0) and got[1][:6] == (33 * 255, 65 * 255, 0, 0, 32, 0) and got[2][:2] == (-1, 19 * 255)
    got, chars, src, parts = check(S, f, sp, rc, pc, first, n_of, full_t, 0, 0, 255)
    assert got[0][0] == 17 * 255 and got[1][0] == 65 * 255
    # the dearest path there is: every atom its own part, read, with a character inserted behind it
    pc[:] = 255
    for r in range(8):
        for i in range(4):
            pc[int(sp["first_piece"][r]) + LD.piece_of(4, i, i + 1)] = 254
    got, chars, src, parts = check(S, f, sp[:8], np.full((8, 65), 255, np.uint8), pc[:72], [0], [8], full_t, 255, 0, 255)
    assert got[0][0] < (1 << 21)


def test_paths_through_the_states_past_the_wave(S, f):
    """Best paths that run through the labels 63 and 64 and lean on the boundary row and column, through pieces."""
    rng = np.random.default_rng(3)
    cuts = [1, 0, 2]
    sp, rc, pc = make_rows(S, rng, np.array(cuts))
    rc[:] = 60
    pc[:] = 9
    B = np.full((66, 66), 200, np.uint8)
    B[65, 64] = B[64, 63] = B[63, 64] = 1
    B[63, 65] = 2
    # ")(" repeated over the six atoms' worth of parts: the rows say nothing, the table alone decides
    got, chars, src, parts = check(S, f, sp, rc, pc, [0], [3], B, 0, 0, 0)
    n = got[0][2]
    assert chars[0, :n].tolist() == ([64, 63] * 3)[:n] and n % 2 == 0
    check(S, f, sp, rc, pc, [0], [3], B, 3, 4, 8)
    # label 64 against label 0, a tie that the smallest state wins, and label 64 alone cheaper
    tie_r, tie_p = np.full((3, 65), 100, np.uint8), np.full((len(pc), 65), 100, np.uint8)
    tie_r[:, 0] = tie_r[:, 64] = 7
    got, chars, src, parts = check(S, f, sp, tie_r, tie_p, [0], [3], np.zeros((66, 66), np.uint8))
    assert chars[0, :3].tolist() == [0, 0, 0]
    tie_r[:, 64] = 6
    got, chars, src, parts = check(S, f, sp, tie_r, tie_p, [0], [3], np.zeros((66, 66), np.uint8))
    assert chars[0, :3].tolist() == [64, 64, 64]
    tie_p[:, 64] = 1                                                  # ... and through the pieces
    got, chars, src, parts = check(S, f, sp, tie_r, tie_p, [0], [3], np.zeros((66, 66), np.uint8), 0, 0, 0)
    assert chars[0, :got[0][2]].tolist() == [64] * 5 and got[0][7] == 5 and parts[3:, 1].tolist() == [2 + LD.piece_of(3, 0, 1), 2 + LD.piece_of(3, 1, 3)]
    # ending on ')' is free and on anything else dear; beginning with '(' likewise; the boundary state kept by DEL
    B = np.zeros((66, 66), np.uint8)
    B[:65, 65] = 90
    B[64, 65] = 0
    B[65, :65] = 90
    B[65, 63] = 0
    flat_r, flat_p = np.full((3, 65), 30, np.uint8), np.full((len(pc), 65), 30, np.uint8)
    flat_r[:, 5] = 10
    got, chars, src, parts = check(S, f, sp, flat_r, flat_p, [0], [3], B, 0, 0, 200)
    assert chars[0, :3].tolist() == [63, 5, 64] and got[0][0] == 30 + 10 + 30
    got, chars, src, parts = check(S, f, sp, flat_r, flat_p, [0], [3], B, 0, 1, 200)
    assert got[0][0] == 3 + int(B[65, 65]) and got[0][4] == 3
    # INS of label 64 behind label 63, and of 63 behind 64, on random rows with those two cheap
    first, n_of = _spans([6, 3, 1, 5])
    sp, rc, pc = make_rows(S, rng, rng.integers(0, 4, 15))
    rc, pc = (100 + rc // 2).astype(np.uint8), (100 + pc // 2).astype(np.uint8)
    rc[:, 63:] = rng.integers(0, 4, (len(rc), 2))
    pc[:, 63:] = rng.integers(0, 4, (len(pc), 2))
    rc[rng.random(len(rc)) < 0.5, 64] = 200                              # (half the rows read '(' alone: "((" needs a ')' put in between)
    pc[rng.random(len(pc)) < 0.5, 64] = 200
    B = rng.integers(100, 256, (66, 66)).astype(np.uint8)
    B[63, 64] = B[64, 63] = B[65, 63] = B[65, 64] = B[63, 65] = B[64, 65] = 0
    got, chars, src, parts = check(S, f, sp, rc, pc, first, n_of, B, 2, 50, 1)
    assert set(chars[0, :got[0][2]].tolist()) <= {63, 64} and sum(g[5] for g in got) > 0


def test_uncut_words_equal_the_word_decoder_on_the_same_rows(S, f):
    rng = np.random.default_rng(4)
    first, n_of = _spans([5, 1, 32, 0, 17, 33, 2])
    sp, rc, pc = make_rows(S, rng, np.zeros(int(n_of.sum()), np.int64))
    rc = cheapen(rng, rc)
    for ins, dele, split in MOVES:
        B = rng.integers(0, 256 if ins else 32, (66, 66)).astype(np.uint8)
        got, chars, src, parts = check(S, f, sp, rc, pc, first, n_of, B, ins, dele, split)
        wdec, wchars, wsrc = f.decode_words(rc, first, n_of)
        assert [g[:6] for g in got] == WD.as_tuples(wdec) and chars.tobytes() == wchars.tobytes() and src.tobytes() == wsrc.tobytes()
        assert parts[:, 0].tolist() == [r for w in range(len(n_of)) if n_of[w] <= 32 for r in range(first[w], first[w] + n_of[w])] and (parts[:, 1] == -1).all()


def test_random_words_and_a_repeat_call(S, f):
    rng = np.random.default_rng(5)
    first, n_of = _spans(rng.integers(0, 17, 60))
    sp, rc, pc = make_rows(S, rng, rng.integers(0, 4, int(n_of.sum())))
    rc, pc = (120 + cheapen(rng, rc) // 2).astype(np.uint8), (cheapen(rng, pc) // 3).astype(np.uint8)          # (dear runs, cheap pieces: cuts pay)
    import word_match_ref as WM
    B = S.bigram_from_words(["".join(rng.choice(list(WM.ALPHABET), int(rng.integers(1, 9)))) for _ in range(300)])
    got, chars, src, parts = check(S, f, sp, rc, pc, first, n_of, B, 64, 250, 8)
    assert any(g[0] < 0 for g in got) and any(g[0] >= 0 and g[7] > n for g, n in zip(got, n_of))
    dec, c2, s2, p2 = f.lattice_decode_words(sp, rc, pc, first, n_of)
    assert LD.as_tuples(dec) == got and c2.tobytes() == chars.tobytes() and s2.tobytes() == src.tobytes() and np.stack([p2["run"], p2["piece"]], 1).tolist() == parts.tolist()
    assert f.lattice_decode_stats() > 0
    # overlapping words are words too
    dec, c3, _, p3 = f.lattice_decode_words(sp, rc, pc, [0, 0, 3], [5, 5, 6])
    assert dec[0][list(dec.dtype.names[:6])] == dec[1][list(dec.dtype.names[:6])] and c3[0].tobytes() == c3[1].tobytes()


def test_errors_leave_the_context_usable(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    try:
        rng = np.random.default_rng(1)
        sp, rc, pc = make_rows(S, rng, np.array([1, 0]))
        assert ctx.lattice_decode_stats() == 0
        with pytest.raises(S.StrErError) as e:                           # no table
            ctx.lattice_decode_words(sp, rc, pc, [0], [2])
        assert e.value.code == -6 and "bigram" in str(e.value)
        assert ctx.lattice_decode_stats() == 0
        B = np.zeros((66, 66), np.uint8)
        B[65, 65] = 3
        ctx.set_bigram(B)
        dec, chars, src, parts = ctx.lattice_decode_words(sp, rc, pc, [0, 0], [2, 0])
        assert LD.as_tuples(dec)[1] == (3, 3, 0, 0, 0, 0, int(dec[0]["n_parts"]), 0)
        for first, n_of in (([1], [2]), ([0], [-1]), ([-1], [1])):
            with pytest.raises(S.StrErError) as e:                       # a word outside the runs
                ctx.lattice_decode_words(sp, rc, pc, first, n_of)
            assert e.value.code == -1
        bad = sp.copy()
        bad["n_cuts"][0] = 4
        with pytest.raises(S.StrErError) as e:
            ctx.lattice_decode_words(bad, rc, pc, [0], [2])
        assert e.value.code == -1
        bad = sp.copy()
        bad["first_piece"][0] = 1
        with pytest.raises(S.StrErError) as e:                           # pieces outside the rows
            ctx.lattice_decode_words(bad, rc, pc, [0], [2])
        assert e.value.code == -1
        # cap_parts too small: STR_ER_ECAPACITY with *n_parts still set
        L = S.load_library()
        import ctypes as C
        fr, no, n = np.zeros(1, np.int32), np.full(1, 2, np.int32), C.c_int32(-5)
        d1, ch, sr, pt = np.zeros(1, S.LATTICE_DECODE_DTYPE), np.zeros(64, np.uint8), np.zeros(64, np.uint8), np.zeros(4, S.SPLIT_PART_DTYPE)
        p = lambda a: a.ctypes.data
        assert L.str_er_lattice_decode_words(ctx.h, p(sp), 2, p(rc), p(pc), len(pc), p(fr), p(no), 1, p(d1), p(ch), p(sr), p(pt), 1, C.byref(n)) == -7
        assert n.value == int(dec[0]["n_parts"]) >= 2
        assert L.str_er_lattice_decode_words(ctx.h, p(sp), 2, p(rc), p(pc), len(pc), p(fr), p(no), 1, None, p(ch), p(sr), p(pt), 4, C.byref(n)) == -1
        again = ctx.lattice_decode_words(sp, rc, pc, [0, 0], [2, 0])
        assert again[0].tobytes() == dec.tobytes() and again[1].tobytes() == chars.tobytes() and again[3].tobytes() == parts.tobytes()
        ctx.set_bigram(None)
        with pytest.raises(S.StrErError) as e:
            ctx.lattice_decode_words(sp, rc, pc, [0], [2])
        assert e.value.code == -6
    finally:
        ctx.close()
