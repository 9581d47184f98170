"""The track match over the members' piece lattices on the GPU (str_er_lattice_match_tracks; the contract is at
str_er_lattice_track_member): every byte of every track record, member record, source and part against the host entry point, then
against the numpy reference (lattice_track_ref.py) with ==, at the kernels' own edges -- tracks of one member for every combination of cut
counts of 1 .. 3 runs against the lattice match of the word, uncut tracks against the track match on the same rows with the node buckets
(8 / 9, 16 / 17, 32 / 33) mixed inside a track, tracks that change the path (uncut / cut) and the bucket from member to member with an
unusable member in the middle, tracks of unusable members and of none, every row slot, a union of bands with a gap, lexicons of one
length around a chunk of 16 groups with padding slots that would win if they counted, 300 members (the strided loops), 65 537 tracks (the
second launch), constant rows where the tie rules decide, the fold, and the errors of the entry point."""
import itertools

import numpy as np
import pytest

import lattice_decode_ref as LD
import lattice_match_ref as LM
import lattice_track_ref as LT
import track_read_ref as TR
import word_match_ref as WM
from test_lattice_decode_abi import cheapen, make_rows

pytestmark = pytest.mark.gpu
SETTINGS = [(True, 64, 64, 2, 8), (False, 3, 200, 1, 8), (True, 1, 1, 0, 0), (False, 255, 255, 31, 255)]          # fold, INS, DEL, band, SPLIT: test_lattice_match.py's


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


def check(S, f, sp, rc, pc, first, n_of, tf, tc, mem, words, fold=True, ins=64, dele=64, band=2, split=8, ref=True, set_lex=True):
    """set_lexicon, set_word_match, set_run_split and lattice_match_tracks against the host entry point (bytes) and, with ref, the numpy
    reference; returns the track records (TRACK_FIELDS) and member records (MEMBER_FIELDS) as tuples, the sources and the parts as (run,
    piece) rows."""
    if set_lex:
        f.set_lexicon(words, fold_case=fold)
    f.set_word_match(ins, dele, band)
    f.set_run_split(1, 4, split)
    rec, mrec, src, parts = f.lattice_match_tracks(sp, rc, pc, first, n_of, tf, tc, mem)
    assert rec.dtype == S.TRACK_MATCH_DTYPE and mrec.dtype == S.LATTICE_TRACK_MEMBER_DTYPE and parts.dtype == S.SPLIT_PART_DTYPE and src.shape == (len(mem), 32)
    hr, hm, hs, hp = S.lattice_match_tracks_host(sp, rc, pc, first, n_of, tf, tc, mem, words, fold, ins, dele, band, split)
    assert rec.tobytes() == hr.tobytes(), [(g, tuple(rec[g]), tuple(hr[g])) for g in range(len(rec)) if rec[g] != hr[g]][:5]
    assert mrec.tobytes() == hm.tobytes(), [(i, tuple(mrec[i]), tuple(hm[i])) for i in range(len(mrec)) if mrec[i] != hm[i]][:5]
    assert src.tobytes() == hs.tobytes() and parts.tobytes() == hp.tobytes()
    got, gm = LT.as_tuples(rec), LT.members_as_tuples(mrec)
    pr = np.stack([parts["run"], parts["piece"]], 1)
    if ref:
        want = LT.match_tracks(sp, rc, pc, first, n_of, tf, tc, mem, WM.Lexicon(words, fold), ins, dele, band, split)
        assert got == want[0], [(g, a, b) for g, (a, b) in enumerate(zip(got, want[0])) if a != b][:5]
        assert gm == want[1], [(i, a, b) for i, (a, b) in enumerate(zip(gm, want[1])) if a != b][:5]
        assert (src == want[2]).all(), np.argwhere(src != want[2])[:5]
        assert pr.tolist() == want[3].tolist()
    for g, (a, n) in zip(got, zip(tf, tc)):                    # what holds for every track
        own = gm[int(a):int(a) + int(n)]
        if g[0] < 0:
            assert g[:4] == (-1, -1, -1, -1) and g[7] == -1 and all(m[0] == -1 and m[2:5] == (0, 0, 0) for m in own)
        else:
            assert sum(m[0] for m in own if m[0] >= 0) == g[1] and sum(1 for m in own if m[0] >= 0) == g[6]
            assert all(m[2] - m[3] + m[4] == len(words[g[0]]) for m in own if m[0] >= 0)
    assert [m[1] for m in gm] == np.concatenate([[0], np.cumsum([m[2] for m in gm])])[:-1].astype(int).tolist() and len(pr) == sum(m[2] for m in gm)
    return got, gm, src, pr


@pytest.mark.parametrize("fold,ins,dele,band,split", SETTINGS)
def test_tracks_of_one_member_for_every_combination_of_cut_counts(S, f, fold, ins, dele, band, split):
    rng = np.random.default_rng(5000 + ins + band)
    combos = [c for R in (1, 2, 3) for c in itertools.product(range(4), repeat=R)]          # 84 words, each a track of one
    first, n_of = _spans([len(c) for c in combos])
    sp, rc, pc = make_rows(S, rng, np.array([k for c in combos for k in c]))
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    words = _words(rng, 150, 1, 9, labels=12) + _words(rng, 10, 10, 14, labels=12)          # (few labels: close costs, and ties)
    nw = len(combos)
    got, gm, src, parts = check(S, f, sp, rc, pc, first, n_of, np.arange(nw), np.ones(nw, np.int32), np.arange(nw), words, fold, ins, dele, band, split, ref=band < 31)
    one, osrc, oparts = f.lattice_match_words(sp, rc, pc, first, n_of)
    assert [g[:6] for g in got] == [r[:6] for r in LM.as_tuples(one)]
    assert src.tobytes() == osrc.tobytes() and parts.tolist() == np.stack([oparts["run"], oparts["piece"]], 1).tolist()
    assert [(m[0] if m[0] >= 0 else -1,) + m[1:5] for m in gm] == [(int(r["cost"]), int(r["first_part"]), int(r["n_parts"]), int(r["n_del"]), int(r["n_ins"])) for r in one]
    if split < 255:
        assert (parts[:, 1] >= 0).any()                        # some member reads a piece


def test_uncut_tracks_equal_the_track_match_on_the_same_rows(S, f):
    """Tracks of 1, 2, 3 and 8 members, the run counts 8 / 9, 16 / 17 and 32 / 33 mixed inside a track."""
    rng = np.random.default_rng(5100)
    first, n_of = _spans([8, 9, 16, 17, 32, 33, 1, 2, 0, 5])
    sp, rc, pc = make_rows(S, rng, np.zeros(int(n_of.sum()), np.int64))
    rc = cheapen(rng, rc)
    mem = [0, 1, 2, 3, 4, 5, 9, 8, 3, 0, 4, 1, 5, 2, 6, 7]
    tf, tc = [0, 1, 3, 6, 8], [1, 2, 3, 2, 8]
    words = _words(rng, 300, 1, 12) + _words(rng, 60, 14, 20, labels=8) + _words(rng, 40, 28, 32, labels=8)
    for fold, band in ((True, 2), (False, 0), (True, 31)):
        got, gm, src, parts = check(S, f, sp, rc, pc, first, n_of, tf, tc, mem, words, fold, 64, 64, band, 8, ref=band < 31)
        plain, mc = f.match_tracks(rc, first, n_of, tf, tc, mem)
        assert got == TR.as_tuples(plain) and [m[0] for m in gm] == mc.tolist()
        runs = [r for i, w in enumerate(mem) if gm[i][0] >= 0 for r in range(first[w], first[w] + n_of[w])]
        assert parts[:, 0].tolist() == runs and (parts[:, 1] == -1).all()


def test_mixed_tracks_change_the_path_and_the_bucket_from_member_to_member(S, f):
    """One track: an uncut member (the matcher's loop), a cut one, then N = 8 -> 32 -> 33 (unusable) -> 16; a track of unusable members
    alone; a track without members; 8 runs of 3 cuts beside 32 uncut runs (every row slot the kernel stages)."""
    rng = np.random.default_rng(5200)
    shapes = [[0, 0, 0], [1, 2], [3, 3], [3] * 8, [3] * 8 + [0], [3] * 4, [0] * 33, [0] * 32, [2, 1] * 3 + [0, 1], []]
    first, n_of = _spans([len(c) for c in shapes])
    sp, rc, pc = make_rows(S, rng, np.array([k for c in shapes for k in c], np.int64))
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    mem = [0, 1, 2, 3, 4, 5, 4, 6, 3, 7, 8, 9, 1]
    tf, tc = [0, 6, 8, 8, 10], [6, 2, 0, 2, 3]
    words = _words(rng, 40, 1, 1) + _words(rng, 40, 32, 32, labels=6) + _words(rng, 200, 2, 31, labels=6)
    for band, ref in ((0, True), (2, True), (31, False)):
        got, gm, src, parts = check(S, f, sp, rc, pc, first, n_of, tf, tc, mem, words, True, 40, 50, band, 8, ref=ref)
        assert got[0][6] == 5 and gm[4][0] == -1 and gm[4][5] == 4 and (src[4] == 255).all()          # the member of 33 nodes in the middle
        assert got[1][:4] == (-1, -1, -1, -1) and got[1][5:] == (0, 0, -1) and got[1][4] > 0          # unusable members alone: nothing tried, free_cost made
        assert got[2] == (-1, -1, -1, -1, 0, 0, 0, -1)                                                 # no members
        assert got[3][0] >= 0 and got[3][6] == 2                                                       # 32 nodes beside 32 nodes: the entries of 32 characters
    # band 31 against the reference on the track of two members of 32 nodes alone
    check(S, f, sp, rc, pc, first, n_of, [8], [2], mem, words[:100], True, 40, 50, 31, 8)


def test_a_union_of_bands_with_a_gap(S, f):
    """Members with (R, N) = (2, 2) and (10, 14) at band 1 try the lengths 1 .. 3 and 9 .. 15.  The label 'x' is free on every row and
    every other label dear: the entries of 4 .. 8 'x' in the gap and of 16 beyond would be the cheapest if they were tried."""
    rng = np.random.default_rng(5300)
    first, n_of = _spans([2, 10])
    sp, rc, pc = make_rows(S, rng, np.array([0, 0] + [1, 1, 1, 1] + [0] * 6))
    rc[:], pc[:] = 200, 200
    rc[:, WM.LABEL_OF["x"]], pc[:, WM.LABEL_OF["x"]] = 0, 0
    words = ["yyy", "y", "y" * 9, "y" * 15, "x" * 4, "x" * 5, "x" * 8, "x" * 16, "yy", "y" * 12]
    got, gm, src, parts = check(S, f, sp, rc, pc, first, n_of, [0], [2], [0, 1], words, False, 1, 1, 1, 0)
    assert got[0][5] == 6 and got[0][0] in (0, 1, 2, 3, 8, 9) and got[0][6] == 2
    f.set_word_match(1, 1, 31)
    wide = f.lattice_match_tracks(sp, rc, pc, first, n_of, [0], [2], [0, 1])[0]
    assert int(wide["n_tried"][0]) == 10 and int(wide["entry"][0]) in (4, 5, 6) and int(wide["cost"][0]) < got[0][1]          # (tried, a gap entry wins)


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_one_length_around_a_chunk_of_16_groups(S, f, n):
    """n entries of 5 characters without the label 0, on rows where the label 0 is free: the padding slots of the last group (all
    label 0) would beat every entry if they counted.  The winner sits in the first group and the runner-up in the last slot -- for
    n > 1024 in another chunk -- and a duplicate of the winner right behind it: the smaller index wins a tie.  The track holds the word
    twice: every cost doubles."""
    rng = np.random.default_rng(5400 + n)
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
    got, gm, src, parts = check(S, f, sp, rc, pc, [0], [3], [0], [2], [0, 0], words, False, 64, 64, 2, 8)
    assert got[0] == (3, 2 * (5 + 16), 4, 2 * (5 + 16), got[0][4], n, 2, 0) and gm[0][2:5] == gm[1][2:5] == (5, 0, 0)
    words[4] = words[0]
    got, gm, src, parts = check(S, f, sp, rc, pc, [0], [3], [0], [2], [0, 0], words, False, 64, 64, 2, 8)
    assert got[0][:4] == (3, 2 * (5 + 16), n - 1, 2 * (6 + 16)) and src[0, :5].tolist() == src[1, :5].tolist() == [0, 1, 2, 3, 4]
    assert parts.tolist() == [[0, 0], [0, 1], [1, -1], [2, 2 + LD.piece_of(3, 0, 2)], [2, 2 + LD.piece_of(3, 2, 3)]] * 2


def test_a_track_of_300_members(S, f):
    """300 members of 2 runs: the 256-stride loop of the band mask and the 64-stride loops of the merge and of the best member.  Two
    members have the same rows, cheaper than every other member's: best_member takes the earlier slot."""
    rng = np.random.default_rng(5500)
    first, n_of = _spans([2] * 300)
    sp, rc, pc = make_rows(S, rng, rng.integers(0, 3, 600))
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    for w in (70, 260):
        sp["n_cuts"][2 * w:2 * w + 2], sp["n_pieces"][2 * w:2 * w + 2] = 0, 0
        rc[2 * w:2 * w + 2] = 0
    mem = np.arange(300)[::-1].copy()                          # (slot order is not word order: word 260 sits in the earlier slot)
    words = _words(rng, 40, 2, 2, labels=10)                   # (two characters: the two members of free rows cost nothing)
    got, gm, src, parts = check(S, f, sp, rc, pc, first, n_of, [0], [300], mem, words, True, 64, 64, 1, 8)
    assert got[0][6] == 300 and got[0][7] == 260 and gm[39][0] == gm[229][0] == min(m[0] for m in gm)
    # the members one slot over a stride: 257 members, and the track beside a second one
    check(S, f, sp, rc, pc, first, n_of, [0, 257], [257, 43], mem, words, True, 64, 64, 1, 8)


def test_65537_tracks_take_a_second_launch(S, f):
    rng = np.random.default_rng(5600)
    first, n_of = _spans([1] * 64)
    sp, rc, pc = make_rows(S, rng, rng.integers(0, 4, 64))
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    words = ["ab", "c", "dEf"]
    nt = 65537
    mem = (np.arange(nt) % 64).astype(np.int32)
    got, gm, src, parts = check(S, f, sp, rc, pc, first, n_of, np.arange(nt), np.ones(nt, np.int32), mem, words, True, 64, 64, 2, 8, ref=False)
    want = LT.match_tracks(sp, rc, pc, first, n_of, np.arange(64), np.ones(64, np.int32), np.arange(64), WM.Lexicon(words, True), 64, 64, 2, 8)
    assert got == [want[0][g % 64] for g in range(nt)]
    assert [(m[0],) + m[2:] for m in gm] == [(want[1][i % 64][0],) + want[1][i % 64][2:] for i in range(nt)]
    assert (src == want[2][mem]).all() and got[65535] == want[0][65535 % 64] and got[65536] == want[0][0]


def test_constant_rows_and_rows_of_255_where_the_tie_rules_decide(S, f):
    rng = np.random.default_rng(5700)
    shapes = [[0], [3], [1, 2], [3] * 8, [0] * 32, [2, 0, 3, 1]]
    first, n_of = _spans([len(c) for c in shapes])
    sp, rc, pc = make_rows(S, rng, np.array([k for c in shapes for k in c]))
    tracks = ([1, 1, 2], [0, 5, 1], [3, 4], [2, 5, 2, 0])
    for mem in tracks:
        Rs, Ns = [len(shapes[w]) for w in mem], [sum(k + 1 for k in shapes[w]) for w in mem]
        lens = sorted({1, max(1, min(Rs) - 1), min(Rs), max(Rs), (min(Rs) + max(Ns)) // 2, min(Ns), max(Ns), min(32, max(Ns) + 2)})
        for value, ins, dele, split in ((3, 3, 3, 0), (0, 1, 1, 0), (7, 7, 7, 7), (255, 255, 255, 255)):
            rc[:], pc[:] = value, value
            for l in lens:                                     # each length in turn as the only entry: every member's own backtrack
                got, gm, src, parts = check(S, f, sp, rc, pc, first, n_of, [0], [len(mem)], mem, ["a" * l], True, ins, dele, 31, split)
                assert got[0][0] == 0 and got[0][7] == mem[min(range(len(mem)), key=lambda i: (gm[i][0], i))]
    # everything at 255, l = N = 32, three members
    rc[:], pc[:] = 255, 255
    words = ["".join(WM.ALPHABET[(7 * t + s) % 65] for t in range(32)) for s in range(3)]
    got, gm, src, parts = check(S, f, sp, rc, pc, first, n_of, [0], [3], [3, 4, 3], words, True, 255, 255, 31, 255)
    assert got[0][:4] == (0, 3 * 32 * 255, 1, 3 * 32 * 255) and got[0][5:] == (3, 3, 3)


def test_the_fold_decides(S, f):
    rng = np.random.default_rng(5800)
    sp, rc, pc = make_rows(S, rng, np.array([0, 1]))
    rc[:], pc[:] = 200, 200
    rc[0, WM.LABEL_OF["A"]] = 0                                # the rows read "AB": upper case where the entry has lower case
    rc[1, WM.LABEL_OF["B"]] = 5
    rc[1, WM.LABEL_OF["q"]] = 90
    words = ["ab", "Aq", "zz"]
    got, _, _, _ = check(S, f, sp, rc, pc, [0], [2], [0], [2], [0, 0], words, True)
    assert got[0][:4] == (0, 10, 1, 180)
    got, _, _, _ = check(S, f, sp, rc, pc, [0], [2], [0], [2], [0, 0], words, False)
    assert got[0][:4] == (1, 180, 0, 512)                      # ("ab" unfolded: both runs dropped and both characters inserted, twice)


def test_no_tracks_slots_of_no_track_and_the_same_call_twice(S, f):
    rng = np.random.default_rng(5900)
    words = _words(rng, 100, 1, 6)
    sp, rc, pc = make_rows(S, rng, np.array([1, 2, 0]))
    f.set_lexicon(words)
    rec, mrec, src, parts = f.lattice_match_tracks(sp, rc, pc, [0], [3], [], [], [])
    assert rec.shape == (0,) and mrec.shape == (0,) and src.shape == (0, 32) and parts.shape == (0,)
    got, gm, src, parts = check(S, f, sp, rc, pc, [0, 0, 3, 1], [0, 3, 0, 1], [1, 4], [2, 1], [3, 0, 1, 2, 3, 1], words, True, 9, 9, 2, 8)
    assert gm[0] == (-1, 0, 0, 0, 0, -1) and gm[3][0] == gm[5][0] == -1 and gm[5][5] == -1 and (src[0] == 255).all()          # the slots of no track
    assert gm[1][2:5] == (0, 0, len(words[got[0][0]])) and src[1, 0] == 0x80                                                 # a word without runs: every character inserted
    a = f.lattice_match_tracks(sp, rc, pc, [0, 0, 3, 1], [0, 3, 0, 1], [1, 4], [2, 1], [3, 0, 1, 2, 3, 1])
    b = f.lattice_match_tracks(sp, rc, pc, [0, 0, 3, 1], [0, 3, 0, 1], [1, 4], [2, 1], [3, 0, 1, 2, 3, 1])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert f.lattice_track_stats() > 0


def test_errors_leave_the_context_usable(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    try:
        rng = np.random.default_rng(6000)
        sp, rc, pc = make_rows(S, rng, np.array([1, 0, 3]))
        call = lambda sp_=sp, first=(0,), n_of=(3,), tf=(0,), tc=(2,), mem=(0, 0): ctx.lattice_match_tracks(sp_, rc, pc, list(first), list(n_of), list(tf), list(tc), list(mem))
        assert ctx.lattice_track_stats() == 0
        with pytest.raises(S.StrErError) as e:                # no lexicon
            call()
        assert e.value.code == -6 and "lexicon" in str(e.value)
        words = _words(rng, 50, 2, 9)
        ctx.set_lexicon(words)
        want = call()
        for first, n_of in (([1], [3]), ([0], [-1]), ([-1], [1])):
            with pytest.raises(S.StrErError) as e:            # a word outside the runs
                call(first=first, n_of=n_of)
            assert e.value.code == -1
        for field, value in (("n_cuts", 4), ("n_pieces", 3), ("first_piece", len(pc) - 1)):
            bad = sp.copy()
            bad[field][0] = value
            with pytest.raises(S.StrErError) as e:            # n_cuts = 4, pieces that do not follow, a piece outside the rows
                call(sp_=bad)
            assert e.value.code == -1
        for mem in ((0, 1), (-1, 0)):
            with pytest.raises(S.StrErError) as e:            # a member outside the words
                call(mem=mem)
            assert e.value.code == -1
        for tf, tc in (((1, 0), (1, 1)), ((0, 0), (1, 1)), ((0,), (3,))):
            with pytest.raises(S.StrErError) as e:            # tracks that do not ascend, that overlap, that leave the member array
                call(tf=tf, tc=tc)
            assert e.value.code == -1
        with pytest.raises(S.StrErError) as e:                # more than 65536 members
            call(tc=(65537,), mem=[0] * 65537)
        assert e.value.code == -7 and "65536" in str(e.value)
        got = call()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
        host = S.lattice_match_tracks_host(sp, rc, pc, [0], [3], [0], [2], [0, 0], words)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, host))
        ctx.set_lexicon([])
        with pytest.raises(S.StrErError) as e:
            call()
        assert e.value.code == -6
    finally:
        ctx.close()
