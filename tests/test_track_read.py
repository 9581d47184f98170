"""The track match on the GPU (str_er_match_tracks; the contract is at str_er_word_link): every field of every record and every member
cost against the numpy reference (track_read_ref.py) with ==, on made-up cost rows at the kernels' own edges -- the buckets of the run
count (8, 16, 32) inside one track, more members than a workgroup stages at once, a chunk of the lexicon, the union of the members'
bands of lengths, the slices of the grid's y."""

import numpy as np
import pytest

import track_read_ref as TR
import word_match_ref as WM
from test_track_read_ref import POOLED_LEXICON, POOLED_ROWS

pytestmark = pytest.mark.gpu
LETTERS = list(WM.ALPHABET)


@pytest.fixture(scope="module")
def f(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    yield ctx
    ctx.close()


def _word(rng, n):
    return "".join(rng.choice(LETTERS, n))


def _rows(rng, n):
    """Random cost rows: a few cheap characters per run among dear ones, so that substitutions, INS and DEL all win somewhere."""
    c = rng.integers(60, 256, (n, 65))
    cheap = rng.random((n, 65)) < 0.08
    c[cheap] = rng.integers(0, 24, int(cheap.sum()))
    return c.astype(np.uint8)


def _spans(n_of):
    n_of = np.asarray(n_of, np.int64)
    return np.concatenate([[0], np.cumsum(n_of)[:-1]]).astype(np.int32), n_of.astype(np.int32)


def check(f, words, costs, n_of, tracks, fold=True, ins=64, dele=64, band=2):
    """set_lexicon, set_word_match and match_tracks against the reference, and what holds for every case: the member costs add up
    to the cost, the best member is the cheapest (the earliest of equals), a track of one is that word's own match, and the same
    call gives the same bytes.  tracks: a list of lists of word indices.  Returns the records as tuples (TRACK_FIELDS)."""
    first, n_of = _spans(n_of)
    tcount = np.array([len(t) for t in tracks], np.int32)
    tfirst = (np.concatenate([[0], np.cumsum(tcount)[:-1]]) if len(tracks) else np.zeros(0)).astype(np.int32)
    members = np.array([w for t in tracks for w in t], np.int32)
    f.set_lexicon(words, fold_case=fold)
    f.set_word_match(ins, dele, band)
    rec, mc = f.match_tracks(costs, first, n_of, tfirst, tcount, members)
    got = TR.as_tuples(rec)
    want, want_mc = TR.match_tracks(costs, first, n_of, tfirst, tcount, members, WM.Lexicon(words, fold), ins, dele, band)
    assert got == want, [(g, a, b) for g, (a, b) in enumerate(zip(got, want)) if a != b][:5]
    assert mc.tolist() == want_mc.tolist()
    alone = WM.as_tuples(f.match_words(costs, first, n_of)) if len(n_of) else []
    for g, t in enumerate(tracks):
        own = mc[tfirst[g]:tfirst[g] + tcount[g]].tolist()
        usable = [i for i, w in enumerate(t) if n_of[w] <= 32]
        assert got[g][6] == len(usable)
        if got[g][0] >= 0:
            assert sum(own[i] for i in usable) == got[g][1] and all(own[i] >= 0 for i in usable)
            assert got[g][7] == t[min(usable, key=lambda i: (own[i], i))]
        else:
            assert got[g][7] == -1 and all(c == -1 for c in own)
        assert all(own[i] == -1 for i in range(len(t)) if i not in usable)
        if len(t) == 1 and usable:
            assert got[g][:6] == alone[t[0]]
    rec2, mc2 = f.match_tracks(costs, first, n_of, tfirst, tcount, members)
    assert rec.tobytes() == rec2.tobytes() and mc.tobytes() == mc2.tobytes()
    return got


def test_pooled_example(f):
    """Two members that each take another entry alone; pooled, the track takes a third."""
    for fold in (True, False):
        got = check(f, POOLED_LEXICON, POOLED_ROWS, [2, 2], [[0, 1], [0], [1]], fold=fold)
        assert got == [(2, 20, 0, 50, 0, 3, 2, 0), (0, 0, 2, 10, 0, 3, 1, 0), (1, 0, 2, 10, 0, 3, 1, 1)]


def test_run_counts_buckets_and_member_counts(f):
    rng = np.random.default_rng(1)
    words = [_word(rng, l) for l in range(1, 33) for _ in range(3)]
    n_of = [0, 1, 8, 9, 16, 17, 32, 33, 40, 5]
    costs = _rows(rng, sum(n_of))
    tracks = [[w] for w in range(len(n_of))]                  # every run count alone: 33 and 40 runs are unusable
    tracks += [[2, 3], [4, 5], [6, 7], [1, 4, 6], [6, 2, 5, 0, 3, 7, 8], [7, 8], [7], []]          # pairs across a bucket's edge, all three buckets, only unusable members, none
    tracks += [[9, 2, 1, 3, 9], [9, 9]]                       # five members; a word twice in one track (and in several tracks)
    tracks += [[int(w) for w in rng.choice([0, 1, 2, 3, 4, 5, 9], 65)]]          # more members than are staged at once, and no multiple of it
    for ins, dele, band in ((64, 64, 2), (40, 90, 1), (64, 64, 0), (64, 64, 31)):
        got = check(f, words, costs, n_of, tracks, ins=ins, dele=dele, band=band)
        assert got[7][:4] == got[15][:4] == got[16][:4] == got[17][:4] == (-1, -1, -1, -1)
        assert got[15][5:] == (0, 0, -1) and got[15][4] > 0 and got[17] == (-1, -1, -1, -1, 0, 0, 0, -1)
        assert got[14][6] == 5 and got[20][6] == 65
    check(f, words, costs, n_of, tracks[10:15], fold=False)


def test_lexicons(f):
    rng = np.random.default_rng(2)
    n_of = [3, 5, 4, 33]
    costs = _rows(rng, sum(n_of))
    tracks = [[0, 1, 2], [1], [3, 0], [2, 2, 1]]
    got = check(f, ["ABCD"], costs, n_of, tracks)             # one entry: no second
    assert all(g[2:4] == (-1, -1) and g[0] == 0 for g in got)
    for l, ms in ((1, [1, 3, 2]), (32, [32, 30, 31])):       # entries of length 1 and of length 32 alone
        check(f, [_word(rng, l) for _ in range(70)], _rows(rng, sum(ms)), ms, [[0, 1, 2], [2, 0], [1]])
    ab = np.full((4, 65), 255, np.uint8)
    ab[[0, 2], WM.LABEL_OF["A"]], ab[[1, 3], WM.LABEL_OF["B"]] = (3, 4), (3, 9)
    got = check(f, ["AB", "CD", "AB"], ab, [2, 2], [[0, 1]])  # duplicates: the lower index wins, the other is second at the same cost
    assert got[0] == (0, 19, 2, 19, 19, 3, 2, 0)
    chunk = f.lexicon_info()["chunk_entries"]
    words = ["".join(rng.choice(list("abcdefghijklmnopqrstuvwxyz"), 4)) for _ in range(chunk + 1)]
    words[chunk], words[7] = "AAAA", "BBBB"                   # one length past a chunk: the best in the second chunk, the second in the first
    reads = np.full((8, 65), 200, np.uint8)
    reads[:4, WM.LABEL_OF["A"]], reads[4:, WM.LABEL_OF["B"]] = 3, 5
    got = check(f, words, reads, [4, 4], [[0, 0, 1], [1, 0]], fold=False)
    assert got[0][:4] == (chunk, 536, 7, 1044) and got[1][:4] == (chunk, 524, 7, 532)
    f.set_lexicon([])                                         # no lexicon
    with pytest.raises(Exception) as e:
        f.match_tracks(costs, [0], [3], [0], [1], [0])
    assert e.value.code == -6 and "lexicon" in str(e.value)


def test_union_of_bands_with_a_gap(f):
    costs = np.zeros((22, 65), np.uint8)
    costs[:, WM.LABEL_OF["B"]] = 255                          # A is free everywhere, B is dear: the entry of ten A would be the cheapest by far
    words = ["A" * 10] + ["B" * l for l in (1, 2, 3, 19, 20, 21, 4, 18, 22)] + ["B" * 2] * 70
    got = check(f, words, costs, [2, 20], [[0, 1], [0], [1]], fold=False, band=1)
    assert got[0][5] == 6 + 70 and got[0][0] != 0 and got[0][0] >= 1          # lengths 1 .. 3 and 19 .. 21 only
    assert got[1][5] == 3 + 70 and got[2][5] == 3
    got = check(f, words, costs, [2, 20], [[0, 1]], fold=False, band=8)       # the bands meet: now the ten A are tried, and win
    assert got[0][0] == 0


def test_no_tracks_and_argument_errors(S, f):
    rng = np.random.default_rng(3)
    f.set_lexicon([_word(rng, 4) for _ in range(10)])
    f.set_word_match()
    costs = _rows(rng, 6)
    rec, mc = f.match_tracks(costs, [0], [6], [], [], [])
    assert rec.shape == (0,) and rec.dtype == S.TRACK_MATCH_DTYPE and mc.shape == (0,)
    rec, mc = f.match_tracks(costs, [0], [6], [1], [1], [0, 0, 0])          # slots of no track stay -1
    assert mc[0] == mc[2] == -1 and mc[1] >= 0
    for tf, tc, mem, code in (([0], [1], [1], -1), ([0], [2], [0], -1), ([0, 0], [1, 1], [0], -1), ([0], [65537], np.zeros(65537, np.int32), -7)):
        with pytest.raises(S.StrErError) as e:
            f.match_tracks(costs, [0], [6], tf, tc, mem)
        assert e.value.code == code
    with pytest.raises(S.StrErError) as e:
        f.match_tracks(costs, [3], [6], [0], [1], [0])                    # a word outside the rows
    assert e.value.code == -1
    for num, den in ((0, 2), (1, 0), (65536, 1), (1, 65536)):
        with pytest.raises(S.StrErError) as e:
            f.set_word_link(num, den)
        assert e.value.code == -1
    f.set_word_link(65535, 65535)
    f.set_word_link()
    want = TR.match_tracks(costs, [0], [6], [0], [1], [0], WM.Lexicon(f._lexicon, True))[0]
    assert TR.as_tuples(f.match_tracks(costs, [0], [6], [0], [1], [0])[0]) == want          # the context is as it was


def test_more_tracks_than_one_launch_takes(f):
    """65537 tracks of one member of one run against three entries: the tracks are the grid's y, at most 65535 a launch."""
    rng = np.random.default_rng(4)
    words = ["A", "BC", "D"]
    costs = _rows(rng, 4)
    costs[0, WM.LABEL_OF["A"]], costs[1, WM.LABEL_OF["D"]], costs[3, WM.LABEL_OF["B"]] = 0, 1, 2
    n = 65537
    members = (np.arange(n) % 4).astype(np.int32)
    f.set_lexicon(words, fold_case=False)
    f.set_word_match()
    rec, mc = f.match_tracks(costs, np.arange(4), np.ones(4), np.arange(n), np.ones(n), members)
    want, want_mc = TR.match_tracks(costs, np.arange(4), np.ones(4), np.arange(4), np.ones(4), np.arange(4), WM.Lexicon(words, False))          # (four different tracks: the reference once)
    assert len({w[0] for w in want}) > 1
    got = TR.as_tuples(rec)
    assert got[:4] == want and got[65532:] == [want[g % 4] for g in range(65532, n)]
    tiled = np.array([w for w in want], np.int64)[members]
    assert (np.array(got, np.int64) == tiled).all() and (mc == want_mc[members]).all()
