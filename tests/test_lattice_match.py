"""The lexicon match over the piece lattice on the GPU (str_er_lattice_match_words; the contract is at str_er_lattice_match): every field
of every record, every source byte and every part against the host entry point (bytes) and the numpy reference (lattice_match_ref.py)
with ==, at the kernels' own edges -- every combination of cut counts of 1 .. 3 runs, N around the node buckets (8 / 9, 16 / 17) and the
limit (32 / 33), 32 uncut runs and 8 runs of 3 cuts (every row slot), entries of 1 and 32 characters, the band's edges, lexicons of one
length around a wave and a chunk with the winner and the runner-up in different chunks and padding slots that would win if they
counted, duplicates, the fold, a run boundary no edge may cross, constant rows where the tie rules decide, everything at 255, and the
uncut words against the matcher on the same rows."""
import itertools

import numpy as np
import pytest

import lattice_decode_ref as LD
import lattice_match_ref as LM
import word_match_ref as WM
from test_lattice_decode_abi import cheapen, make_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def f(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    yield ctx
    ctx.close()


def _spans(n_of):
    n_of = np.asarray(n_of, np.int64)
    return np.concatenate([[0], np.cumsum(n_of)])[:len(n_of)].astype(np.int32), n_of.astype(np.int32)


def _words(rng, n, lo, hi, labels=65):
    return ["".join(WM.ALPHABET[a] for a in rng.integers(65 - labels, 65, int(l))) for l in rng.integers(lo, hi + 1, n)]


def check(S, f, sp, rc, pc, first, n_of, words, fold=True, ins=64, dele=64, band=2, split=8, ref=True, set_lex=True):
    """set_lexicon, set_word_match, set_run_split and lattice_match_words against the host entry point (bytes) and, with ref, the numpy
    reference; returns the records as tuples (MATCH_FIELDS), the sources and the parts as (run, piece) rows."""
    if set_lex:
        f.set_lexicon(words, fold_case=fold)
    f.set_word_match(ins, dele, band)
    f.set_run_split(1, 4, split)
    rec, src, parts = f.lattice_match_words(sp, rc, pc, first, n_of)
    assert rec.dtype == S.LATTICE_MATCH_DTYPE and parts.dtype == S.SPLIT_PART_DTYPE and src.shape == (len(first), 32)
    hr, hs, hp = S.lattice_match_words_host(sp, rc, pc, first, n_of, words, fold, ins, dele, band, split)
    assert rec.tobytes() == hr.tobytes() and src.tobytes() == hs.tobytes() and parts.tobytes() == hp.tobytes(), \
        [(w, tuple(rec[w]), tuple(hr[w])) for w in range(len(rec)) if rec[w] != hr[w] or (src[w] != hs[w]).any()][:5]
    got = LM.as_tuples(rec)
    pr = np.stack([parts["run"], parts["piece"]], 1)
    if ref:
        want = LM.match_words(sp, rc, pc, first, n_of, WM.Lexicon(words, fold), ins, dele, band, split)
        assert got == want[0], [(w, g, x) for w, (g, x) in enumerate(zip(got, want[0])) if g != x][:5]
        assert (src == want[1]).all(), np.argwhere(src != want[1])[:5]
        assert pr.tolist() == want[2].tolist()
    for g in got:                                              # what holds for every record
        if g[0] < 0:
            assert g[:4] == (-1, -1, -1, -1) and g[7:] == (0, 0, 0)
        else:
            assert g[7] - g[8] + g[9] == len(words[g[0]]) and g[1] >= 0
    assert [g[6] for g in got] == np.concatenate([[0], np.cumsum([g[7] for g in got])])[:-1].astype(int).tolist()
    return got, src, pr


@pytest.mark.parametrize("fold,ins,dele,band,split", [(True, 64, 64, 2, 8), (False, 3, 200, 1, 8), (True, 1, 1, 0, 0), (False, 255, 255, 31, 255)])
def test_every_combination_of_cut_counts_of_one_to_three_runs(S, f, fold, ins, dele, band, split):
    rng = np.random.default_rng(3000 + ins + band)
    combos = [c for R in (1, 2, 3) for c in itertools.product(range(4), repeat=R)]          # 84 words
    first, n_of = _spans([len(c) for c in combos])
    sp, rc, pc = make_rows(S, rng, np.array([k for c in combos for k in c]))
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    words = _words(rng, 150, 1, 9, labels=12) + _words(rng, 10, 10, 14, labels=12)          # (few labels: close costs, and ties)
    got, src, parts = check(S, f, sp, rc, pc, first, n_of, words, fold, ins, dele, band, split, ref=band < 31)
    assert all(g[0] >= 0 for g in got) or band == 0
    if split < 255:
        assert (parts[:, 1] >= 0).any()                        # some winner reads a piece


def test_node_buckets_the_limit_and_every_row_slot(S, f):
    """N = 8 / 9 and 16 / 17 (the buckets), 32 / 33 (the limit); 32 uncut runs and 8 runs of 3 cuts (80 edge rows: every slot the
    kernel stages); entries of 1 and 32 characters; band 0 and 31."""
    rng = np.random.default_rng(3100)
    shapes = [[3, 3], [3, 3, 0], [3] * 4, [3] * 4 + [0], [3] * 8, [3] * 8 + [0], [0] * 32, [0] * 33, [0] * 8, [0] * 9, [1] * 8, [2, 1] * 3 + [0, 1], [0] * 31 + [1]]
    first, n_of = _spans([len(c) for c in shapes])
    sp, rc, pc = make_rows(S, rng, np.array([k for c in shapes for k in c]))
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    words = _words(rng, 40, 1, 1) + _words(rng, 40, 32, 32, labels=6) + _words(rng, 200, 2, 31, labels=6)
    for band, ref in ((0, True), (31, False), (2, True)):
        got, src, parts = check(S, f, sp, rc, pc, first, n_of, words, True, 40, 50, band, 8, ref=ref)
        for w in (5, 7, 12):                                   # N = 33: nothing tried, free_cost still made
            assert got[w][:4] == (-1, -1, -1, -1) and got[w][5] == 0 and got[w][4] > 0 and (src[w] == 255).all()
        assert got[4][0] >= 0 and got[6][0] >= 0               # N = 32 is tried at every band: the entries of 32 characters
    # band 31 against the reference on the two words of 32 nodes alone (every length is tried: the reference takes a while per word)
    sel = np.array([4, 6])
    check(S, f, sp, rc, pc, first[sel], n_of[sel], words[:120], True, 40, 50, 31, 8)


def test_the_edges_of_the_band(S, f):
    """A word of R = 3 runs and N = 6 atoms under band 1: the lengths R - band - 1, R - band, N + band, N + band + 1 = 1, 2, 7, 8."""
    rng = np.random.default_rng(3200)
    sp, rc, pc = make_rows(S, rng, np.array([1, 0, 2]))
    words = _words(rng, 5, 1, 1) + _words(rng, 6, 2, 2) + _words(rng, 7, 7, 7) + _words(rng, 9, 8, 8)
    got, _, _ = check(S, f, sp, rc, pc, [0], [3], words, True, 64, 64, 1, 8)
    assert got[0][5] == 13 and 5 <= got[0][0] < 18
    got, _, _ = check(S, f, sp, rc, pc, [0], [3], words, True, 64, 64, 0, 8)
    assert got[0][5] == 0 and got[0][0] == -1                  # (lengths 3 .. 6: none in this lexicon)
    got, _, _ = check(S, f, sp, rc, pc, [0], [3], words, True, 64, 64, 2, 8)
    assert got[0][5] == 27


@pytest.mark.parametrize("n", [63, 64, 65, 4095, 4096, 4097])
def test_one_length_around_a_wave_and_a_chunk(S, f, n):
    """n entries of 5 characters without the label 0, on rows where the label 0 is free: the padding slots of the last group (all
    label 0) would beat every entry if they counted.  The winner sits in the first group and the runner-up in the last slot -- for
    n > 4096 in another chunk -- and a duplicate of the winner right behind it: the smaller index wins a tie."""
    rng = np.random.default_rng(3300 + n)
    cuts = np.array([1, 0, 2])
    sp, rc, pc = make_rows(S, rng, cuts)
    rc[:], pc[:] = rng.integers(60, 256, rc.shape), rng.integers(60, 256, pc.shape)
    rc[:, 0], pc[:, 0] = 0, 0
    E = rng.integers(1, 65, (n, 5))
    E[3] = [11, 22, 33, 44, 55]
    E[4] = E[3]                                                # the duplicate
    E[n - 1] = [11, 22, 33, 44, 56]
    # the path: piece (0, 1) and (1, 2) of run 0, run 1 whole, piece (0, 2) and (2, 3) of run 2
    for r, i, j, a in ((0, 0, 1, 11), (0, 1, 2, 22), (1, 0, 1, 33), (2, 0, 2, 44), (2, 2, 3, 55)):
        k = LD.piece_of(int(cuts[r]) + 1, i, j)
        (rc[r] if k < 0 else pc[int(sp["first_piece"][r]) + k])[a] = 1
    pc[int(sp["first_piece"][2]) + LD.piece_of(3, 2, 3), 56] = 2
    words = ["".join(WM.ALPHABET[a] for a in e) for e in E]
    got, src, parts = check(S, f, sp, rc, pc, [0], [3], words, False, 64, 64, 2, 8)
    assert got[0][:4] == (3, 5 + 16, 4, 5 + 16) and got[0][5] == n and got[0][7:] == (5, 0, 0)
    words[4] = words[0]
    got, src, parts = check(S, f, sp, rc, pc, [0], [3], words, False, 64, 64, 2, 8)
    assert got[0][:4] == (3, 5 + 16, n - 1, 6 + 16) and src[0, :5].tolist() == [0, 1, 2, 3, 4]
    assert parts.tolist() == [[0, 0], [0, 1], [1, -1], [2, 2 + LD.piece_of(3, 0, 2)], [2, 2 + LD.piece_of(3, 2, 3)]]


def test_the_fold_decides(S, f):
    rng = np.random.default_rng(3400)
    sp, rc, pc = make_rows(S, rng, np.array([0, 1]))
    rc[:], pc[:] = 200, 200
    rc[0, WM.LABEL_OF["A"]] = 0                                # the rows read "AB" / "A" + "b" "C": upper case where the entry has lower case
    rc[1, WM.LABEL_OF["B"]] = 5
    rc[1, WM.LABEL_OF["q"]] = 90
    words = ["ab", "Aq", "zz"]
    got, _, _ = check(S, f, sp, rc, pc, [0], [2], words, True)
    assert got[0][:4] == (0, 5, 1, 90)
    got, _, _ = check(S, f, sp, rc, pc, [0], [2], words, False)
    assert got[0][:4] == (1, 90, 0, 256)                       # ("ab" unfolded: both runs dropped and both characters inserted)


def test_no_edge_crosses_a_run_boundary(S, f):
    """Every edge that ends at the last node of a run or leaves the first node of the next costs 100 whatever it reads, every other
    piece nothing: a legal path pays at least 200 to pass the boundary.  A predecessor read across the boundary, or the neighbouring
    run's piece row at this run's slot, would pass it for less."""
    rng = np.random.default_rng(3500)
    for cuts in ([3, 3], [3, 1, 3], [2, 3, 3, 2], [1, 3] * 4):
        sp, rc, pc = make_rows(S, rng, np.array(cuts))
        rc[:], pc[:] = 100, 0
        for r, k in enumerate(cuts):
            A, fp = k + 1, int(sp["first_piece"][r])
            for i in range(A):
                for j in range(i + 1, A + 1):
                    if (i, j) != (0, A) and (j == A and r + 1 < len(cuts) or i == 0 and r > 0):
                        pc[fp + LD.piece_of(A, i, j)] = 100
        N = sum(k + 1 for k in cuts)
        words = _words(rng, 30, len(cuts), N) + _words(rng, 30, max(1, len(cuts) - 2), N + 2)
        for ins, dele, split in ((255, 255, 1), (30, 40, 0), (1, 1, 8)):
            got, _, _ = check(S, f, sp, rc, pc, [0], [len(cuts)], words, True, ins, dele, 2, split)
            if (ins, dele) == (255, 255):
                assert got[0][1] >= 100 * len(cuts)            # (every run pays at least one dear edge, both neighbours' at a boundary)


def test_constant_rows_where_every_tie_rule_decides(S, f):
    rng = np.random.default_rng(3600)
    for cuts in ([0], [3], [1, 2], [3] * 8, [0] * 32, [2, 0, 3, 1]):
        sp, rc, pc = make_rows(S, rng, np.array(cuts))
        R, N = len(cuts), sum(k + 1 for k in cuts)
        words = sorted({"a" * l for l in (1, max(1, R - 1), R, (R + N) // 2, N, min(32, N + 1), min(32, N + 2))}, key=len)
        for value, ins, dele, split in ((3, 3, 3, 0), (0, 1, 1, 0), (7, 7, 7, 7), (255, 255, 255, 255)):
            rc[:], pc[:] = value, value
            for k in range(len(words)):                       # each length in turn as the only entry: its own backtrack
                got, src, parts = check(S, f, sp, rc, pc, [0], [R], words[k:k + 1], True, ins, dele, 31, split)
                assert got[0][0] == 0


def test_everything_at_255(S, f):
    sp, rc, pc = make_rows(S, np.random.default_rng(1), np.array([3] * 8))
    rc[:], pc[:] = 255, 255
    words = ["".join(WM.ALPHABET[(7 * t + s) % 65] for t in range(32)) for s in range(3)]          # l = N = 32
    got, src, parts = check(S, f, sp, rc, pc, [0], [8], words, True, 255, 255, 31, 255)
    assert got[0][:4] == (0, 32 * 255, 1, 32 * 255) and got[0][4] == 8 * 255 and got[0][5] == 3


def test_uncut_words_equal_the_matcher_on_the_same_rows(S, f):
    rng = np.random.default_rng(3700)
    first, n_of = _spans([0, 1, 2, 5, 8, 9, 16, 17, 32, 33, 3, 4])
    sp, rc, pc = make_rows(S, rng, np.zeros(int(n_of.sum()), np.int64))
    rc = cheapen(rng, rc)
    words = _words(rng, 400, 1, 12) + _words(rng, 40, 28, 32)
    for fold, band in ((True, 2), (False, 0), (True, 31)):
        got, src, parts = check(S, f, sp, rc, pc, first, n_of, words, fold, 64, 64, band, 8, ref=band < 31)
        plain = f.match_words(rc, first, n_of)
        assert [g[:6] for g in got] == WM.as_tuples(plain)
        runs = [r for w in range(len(first)) if got[w][0] >= 0 for r in range(first[w], first[w] + n_of[w])]
        assert parts[:, 0].tolist() == runs and (parts[:, 1] == -1).all()


def test_no_words_words_without_runs_and_the_same_call_twice(S, f):
    rng = np.random.default_rng(3800)
    words = _words(rng, 100, 1, 6)
    f.set_lexicon(words)
    rec, src, parts = f.lattice_match_words(np.zeros(0, S.RUN_SPLIT_DTYPE), np.zeros((0, 65), np.uint8), np.zeros((0, 65), np.uint8), [], [])
    assert rec.shape == (0,) and rec.dtype == S.LATTICE_MATCH_DTYPE and src.shape == (0, 32) and parts.shape == (0,)
    sp, rc, pc = make_rows(S, rng, np.array([1, 2, 0]))
    got, src, parts = check(S, f, sp, rc, pc, [0, 0, 3, 1], [0, 3, 0, 1], words, True, 9, 9, 2, 8)
    assert got[0][:6] == got[2][:6]
    assert got[0][7:] == (0, 0, len(words[got[0][0]])) and src[0, 0] == 0x80
    a = f.lattice_match_words(sp, rc, pc, [0, 0, 3, 1], [0, 3, 0, 1])
    b = f.lattice_match_words(sp, rc, pc, [0, 0, 3, 1], [0, 3, 0, 1])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert f.lattice_match_stats() > 0


def test_errors_leave_the_context_usable(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    try:
        rng = np.random.default_rng(3900)
        sp, rc, pc = make_rows(S, rng, np.array([1, 0, 3]))
        assert ctx.lattice_match_stats() == 0
        with pytest.raises(S.StrErError) as e:                # no lexicon
            ctx.lattice_match_words(sp, rc, pc, [0], [3])
        assert e.value.code == -6 and "lexicon" in str(e.value)
        words = _words(rng, 50, 2, 9)
        ctx.set_lexicon(words)
        want = ctx.lattice_match_words(sp, rc, pc, [0], [3])
        for first, n_of in (([1], [3]), ([0], [-1]), ([-1], [1])):
            with pytest.raises(S.StrErError) as e:            # a word outside the runs
                ctx.lattice_match_words(sp, rc, pc, first, n_of)
            assert e.value.code == -1
        for field, value in (("n_cuts", 4), ("n_pieces", 3), ("first_piece", len(pc) - 1)):
            bad = sp.copy()
            bad[field][0] = value
            with pytest.raises(S.StrErError) as e:            # bad records
                ctx.lattice_match_words(bad, rc, pc, [0], [3])
            assert e.value.code == -1
        got = ctx.lattice_match_words(sp, rc, pc, [0], [3])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
        host = S.lattice_match_words_host(sp, rc, pc, [0], [3], words)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, host))
        ctx.set_lexicon([])
        with pytest.raises(S.StrErError) as e:
            ctx.lattice_match_words(sp, rc, pc, [0], [3])
        assert e.value.code == -6
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_word_counts_around_a_block_of_the_final_kernel(S, f, n):
    rng = np.random.default_rng(4000 + n)
    first, n_of = _spans(rng.integers(0, 5, n))
    sp, rc, pc = make_rows(S, rng, rng.integers(0, 4, int(n_of.sum())))
    words = _words(rng, 90, 1, 7, labels=10)
    got, src, parts = check(S, f, sp, cheapen(rng, rc), cheapen(rng, pc), first, n_of, words, True, 20, 30, 1, 8, ref=n <= 2)
    assert len(got) == n
