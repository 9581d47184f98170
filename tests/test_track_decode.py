"""The track decode on the GPU (str_er_set_track_decode, str_er_decode_tracks; the contract is at str_er_track_decode): every field of
every record, every label and every member cost against the host entry point (str_er_decode_tracks_host) byte for byte and against
the numpy reference (track_decode_ref.py, the full recurrence for every neighbour) with ==, at the kernel's own edges: the lengths 1, 2,
31 and 32 where DEL and INS switch off, row counts of 0 .. 33 mixed inside a track, tracks of no, one and unusable members, a word
listed twice, more usable members than seeds, decoder strings that are no seeds, the strided member loops, the member limit, inputs on
which only (J, index) decides, and the ends of the parameter ranges."""
import numpy as np
import pytest

import track_decode_ref as TD
import word_decode_ref as WD
from test_track_decode_ref import make_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def f(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    yield ctx
    ctx.close()


def pack(words, tracks, gap=0):
    """words: (m, 65) row arrays; tracks: lists of word indices; gap: slots of no track between two tracks (they hold word 0)."""
    n_of = np.array([len(C) for C in words], np.int32)
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]]).astype(np.int32)
    costs = np.concatenate([np.asarray(C, np.uint8).reshape(-1, 65) for C in words] + [np.zeros((0, 65), np.uint8)])
    tf, members = [], []
    for t in tracks:
        tf.append(len(members))
        members += list(t) + [0] * gap
    return costs, first, n_of, np.array(tf, np.int32), np.array([len(t) for t in tracks], np.int32), np.array(members, np.int32)


def check(S, f, packed, B, dec=(0, 0), ins=64, dele=64, rounds=8, ref=True):
    """decode_tracks against decode_tracks_host and (ref) the reference; returns the records as tuples (DECODE_FIELDS), chars, costs."""
    f.set_bigram(B)
    f.set_word_decode(*dec)
    f.set_track_decode(ins, dele, rounds)
    got, ch, mc = f.decode_tracks(*packed)
    host, hch, hmc = S.decode_tracks_host(*packed, B, dec[0], dec[1], ins, dele, rounds)
    recs = TD.as_tuples(got)
    assert recs == TD.as_tuples(host), [(g, a, b) for g, (a, b) in enumerate(zip(recs, TD.as_tuples(host))) if a != b][:5]
    assert got.tobytes() == host.tobytes() and ch.tobytes() == hch.tobytes() and mc.tobytes() == hmc.tobytes()
    if ref:
        want, wch, wmc, _ = TD.decode_tracks(*packed, B, dec[0], dec[1], ins, dele, rounds)
        assert recs == want, [(g, a, b) for g, (a, b) in enumerate(zip(recs, want)) if a != b][:5]
        assert (ch == wch).all() and mc.tolist() == wmc.tolist()
    return recs, ch, mc


def confident(labels, rng, lo=120):
    """Rows that read `labels`: the label costs 0 .. 9, every other character lo .. 255."""
    C = rng.integers(lo, 256, (len(labels), 65))
    C[np.arange(len(labels)), labels] = rng.integers(0, 10, len(labels))
    return C.astype(np.uint8)


def test_the_recipe_under_every_setting(S, f):
    B, packed = make_case()
    for dec, rounds in (((0, 0), 0), ((0, 0), 1), ((0, 0), 64), ((64, 64), 8)):
        recs, _, _ = check(S, f, packed, B, dec, 64, 64, rounds)
        assert all(r[0] >= 0 for r in recs)
    assert any(r[3] >= 2 for r in recs) and any(r[3] == 0 and r[4] == 1 for r in recs)
    for ins, dele in ((1, 1), (255, 255), (1, 255), (255, 1)):
        check(S, f, packed[:3] + (packed[3][:5], packed[4][:5], packed[5]), B, (0, 0), ins, dele, 8)


def test_lengths_where_del_and_ins_switch_off(S, f):
    rng = np.random.default_rng(31)
    B = rng.integers(0, 40, (66, 66)).astype(np.uint8)
    T = [int(a) for a in rng.integers(0, 65, 32)]
    words = [confident(T[:1], rng), confident(T[:1], rng), confident(T[:2], rng)]              # 0 .. 2: l = 1 and 2
    words += [confident(T[:2], rng), confident(T[:2], rng), confident(T[:1], rng)]             # 3 .. 5
    words += [confident(T, rng) for _ in range(3)] + [confident(T[:31], rng)]                  # 6 .. 9: l = 32 and 31
    words += [confident(T[:31], rng) for _ in range(3)] + [confident(T, rng)]                  # 10 .. 13
    tracks = [[0, 1], [2, 0, 1], [3, 4, 5], [6, 7, 8], [9, 6, 7, 8], [13, 10, 11, 12], [10, 11]]
    for rounds in (0, 8):
        recs, ch, _ = check(S, f, pack(words, tracks), B, (0, 0), 64, 64, rounds)
    assert [r[2] for r in recs] == [1, 1, 2, 32, 32, 31, 31]                                  # a DEL from 2 and from 32, an INS to 32 were open
    assert recs[1][3] >= 1 or recs[1][6] != 2
    assert (ch[3] == T).all() and (ch[5, :31] == T[:31]).all()


def test_row_counts_mixed_inside_a_track(S, f):
    rng = np.random.default_rng(32)
    B = rng.integers(0, 120, (66, 66)).astype(np.uint8)
    ms = [0, 1, 8, 9, 16, 17, 32, 33]
    words = [rng.integers(0, 256, (m, 65)).astype(np.uint8) for m in ms] + [confident([3, 4, 5], rng)]
    tracks = [list(range(8)), [7, 6, 5, 4, 3, 2, 1, 0], [0, 7, 8], [6, 8], [1, 2, 8, 8]]
    for dec in ((0, 0), (64, 64)):
        recs, _, mc = check(S, f, pack(words, tracks, gap=2), B, dec, 64, 64, 3)
        assert [r[5] for r in recs] == [7, 7, 2, 2, 4] and mc[7] == -1 and mc[8] == mc[9] == -1 and mc[10] == -1


def test_special_tracks(S, f):
    rng = np.random.default_rng(33)
    B = rng.integers(0, 120, (66, 66)).astype(np.uint8)
    words = [confident([1, 2, 3], rng), rng.integers(0, 256, (33, 65)).astype(np.uint8), rng.integers(0, 256, (40, 65)).astype(np.uint8),
             confident([1, 9, 3, 4], rng), np.zeros((0, 65), np.uint8)]
    tracks = [[], [0], [1, 2], [3, 3, 0], [4], [1, 0]]          # none, one, unusable only, a word twice, a word of no rows, unusable first
    recs, ch, mc = check(S, f, pack(words, tracks, gap=1), B)
    assert recs[0] == (-1, -1, 0, 0, 0, 0, -1, -1) and recs[2] == (-1, -1, 0, 0, 0, 0, -1, -1) and recs[4] == (-1, -1, 0, 0, 0, 1, -1, -1)
    assert (ch[0] == 255).all() and (ch[2] == 255).all() and recs[1][5:7] == (1, 0) and recs[3][5] == 3 and recs[5][5:7] == (1, 0)
    dec, _, _ = f.decode_words(*pack(words, tracks)[:3])
    assert recs[1][1] <= int(dec[0]["cost"])                      # property 5: one usable member, the decoder's INS = DEL = 0
    one, _, _ = check(S, f, pack(words, [[3]]), B)
    two, _, _ = check(S, f, pack(words, [[3, 3]]), B, rounds=0)
    assert two[0][1] == 2 * one[0][1] - TD.lm(WD.decode_word(words[3], B)[1], B)          # it counts twice


def test_the_33rd_member_is_no_seed(S, f):
    B = np.full((66, 66), 10, np.uint8)
    A, Z = [5, 6, 7], [40, 41, 42]
    first32 = np.full((3, 65), 200, np.uint8)
    first32[np.arange(3), A] = 0
    first32[np.arange(3), Z] = 1
    last = np.full((3, 65), 255, np.uint8)
    last[np.arange(3), Z] = 0
    words = [first32] * 32 + [last]
    packed = pack(words, [list(range(33)), [32] + list(range(32))])
    recs, ch, _ = check(S, f, packed, B, rounds=0)
    assert list(ch[0, :3]) == A and recs[0][5] == 33 and 0 <= recs[0][6] < 32
    rows = [words[i] for i in range(33)]
    assert TD.score(rows, Z, B, 64, 64) < recs[0][1] == TD.score(rows, A, B, 64, 64)          # Z would win if it were a seed
    assert list(ch[1, :3]) == Z and recs[1][6] == 32                                             # ... and wins where it is one
    recs, ch, _ = check(S, f, packed, B, rounds=8)
    assert list(ch[0, :3]) == Z and recs[0][3] == 3 and recs[0][4] == 1                           # the polish finds it by three SUBs


def test_decoder_strings_that_are_no_seeds(S, f):
    rng = np.random.default_rng(35)
    x = 64
    B = np.full((66, 66), 200, np.uint8)          # any two characters in a row are dear, but x between them is free: the decoder inserts
    B[:, x] = 0
    B[x, :] = 0
    B[65, :] = 0
    B[:, 65] = 0
    long_, short = confident(list(rng.integers(0, 60, 20)), rng), confident(list(rng.integers(0, 60, 10)), rng)
    dear = np.full((3, 65), 255, np.uint8)
    words = [long_, np.zeros((0, 65), np.uint8), dear, short]
    packed = pack(words, [[0, 1, 2, 3], [0, 1, 2], [3, 0]])
    dec, dch, _ = S.decode_words_host(*packed[:3], B, 1, 200)          # (dropping a row of 255s for 200 pays, dropping a good one does not)
    assert [int(d["n_chars"]) for d in dec] == [39, 0, 0, 19]          # more than 32, none (no rows), none (all dropped), a seed
    for rounds in (0, 2):
        recs, ch, mc = check(S, f, packed, B, (1, 200), 64, 64, rounds)
        assert recs[0][5:7] == (4, 3) and recs[1] == (-1, -1, 0, 0, 0, 3, -1, -1) and recs[2][5:7] == (2, 3)
        assert mc[4:7].tolist() == [-1, -1, -1]
    recs, ch, _ = check(S, f, packed, B, (1, 200), 64, 64, 0)
    assert (ch[0, :19] == dch[3, :19]).all() and recs[0][2] == 19


def test_many_members(S, f):
    rng = np.random.default_rng(36)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    T = [7, 30, 52]
    words = [confident(T[:int(rng.integers(1, 4))], rng, lo=40) for _ in range(300)] + [rng.integers(0, 256, (33, 65)).astype(np.uint8)]
    tracks = [list(range(300)), [300] + list(range(299, -1, -1)), list(range(0, 300, 7))]
    recs, _, _ = check(S, f, pack(words, tracks), B, rounds=2)
    assert [r[5] for r in recs] == [300, 300, 43]
    # the member limit: 1024 are decoded, 1025 are refused by both entry points
    one = [confident([9], rng, lo=40) for _ in range(8)]
    recs, _, mc = check(S, f, pack(one, [[i % 8 for i in range(1024)]]), B, rounds=1)
    assert recs[0][5] == 1024 and (mc >= 0).all()
    packed = pack(one, [[i % 8 for i in range(1025)]])
    for call in (lambda: f.decode_tracks(*packed), lambda: S.decode_tracks_host(*packed, B)):
        with pytest.raises(S.StrErError) as e:
            call()
        assert e.value.code == -7


def test_only_the_index_decides(S, f):
    words = [np.full((m, 65), 7, np.uint8) for m in (2, 3, 4, 3)]
    packed = pack(words, [[0, 1, 2], [1, 3], [2, 0]])
    for B in (np.zeros((66, 66), np.uint8), np.full((66, 66), 255, np.uint8)):
        for ins, dele in ((64, 64), (1, 1), (255, 255)):
            for rounds in (0, 1, 64):
                recs, ch, _ = check(S, f, packed, B, (0, 0), ins, dele, rounds)
                assert (ch[ch != 255] == 0).all()          # every row's first arg min, and no SUB ever pays
    recs, _, _ = check(S, f, packed, np.zeros((66, 66), np.uint8), (0, 0), 1, 1, 64)
    # two members of three rows, INS = DEL = 1 below the rows' 7: a string of l labels costs 2 * (3 + l) unaligned, the seed "000" 12, and
    # the first DEL (index 2080) is taken twice, down to the one label that has to stay
    assert recs[1][:5] == (8, 12, 1, 2, 1)


def test_no_tracks_and_no_table(S, f):
    rng = np.random.default_rng(37)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    words = [confident([1, 2], rng)]
    recs, ch, mc = check(S, f, pack(words, []), B)
    assert recs == [] and ch.shape == (0, 32) and mc.shape == (0,)
    got, ch, mc = f.decode_tracks(np.zeros((0, 65), np.uint8), [], [], [], [], [])
    assert got.shape == (0,) and got.dtype == S.TRACK_DECODE_DTYPE
    f.set_bigram(None)
    with pytest.raises(S.StrErError) as e:
        f.decode_tracks(*pack(words, [[0]]))
    assert e.value.code == -6
    f.set_bigram(B)
    for bad in ((0, 64, 8), (64, 0, 8), (256, 64, 8), (64, 64, 65), (64, 64, -1)):
        with pytest.raises(S.StrErError):
            f.set_track_decode(*bad)
    recs, _, _ = check(S, f, pack(words, [[0]]), B, rounds=8)          # the context is unchanged by the refused setters
    assert recs[0][5] == 1
