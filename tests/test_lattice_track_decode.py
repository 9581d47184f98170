"""The track decode over the members' piece lattices on the GPU (str_er_lattice_decode_tracks; the contract is at
str_er_lattice_track_decode): every record, label, member record, source byte and part against the host entry point
(str_er_lattice_decode_tracks_host) byte for byte, and on the small cases against the numpy reference (lattice_track_decode_ref.py, the
full lattice recurrence for every neighbour) with ==, at the kernel's own edges: every combination of cut counts in words of one and two
runs under the ends of every parameter, the lengths 1, 2, 31 and 32 where DEL and INS switch off, N = 0, 32 and 33 mixed in a track, a
word listed twice, more usable members than seeds, lattice decoder strings that are no seeds, tracks of none and of unusable members,
slots of no track, both sides of the resident-rows limit (512 edges), the strided member loops, the member limit, inputs on which only
(J, index) and the first-candidate rule decide, 65 tracks in a call, and the refusals."""
import itertools

import numpy as np
import pytest

import lattice_decode_ref as LD
import lattice_track_decode_ref as R
import track_decode_ref as TD
from test_lattice_track_decode_ref import make_case

pytestmark = pytest.mark.gpu

RES_EDGES = 512          # (lattice_track_decode_kernels.hip: LTD_RES_EDGES)


@pytest.fixture(scope="module")
def f(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    yield ctx
    ctx.close()


def run(k, row, pieces=None, rng=None, hi=256):
    """A run of k cuts: (k, its row, its piece rows); pieces None: random rows."""
    if pieces is None:
        pieces = [rng.integers(0, hi, 65) for _ in range(LD.n_pieces(k))]
    assert len(pieces) == LD.n_pieces(k)
    return (k, np.asarray(row), pieces)


def word(rng, cuts, hi=256):
    """A word of random rows with the given cut counts; a tenth of the bytes are cheap."""
    def rows(n):
        r = rng.integers(0, hi, (n, 65))
        return np.where(rng.random(r.shape) < 0.1, r // 8, r)
    return [run(k, rows(1)[0], list(rows(LD.n_pieces(k)))) for k in cuts]


def plain(C):
    """(m, 65) rows as a word without cuts."""
    return [run(0, r, []) for r in np.asarray(C).reshape(-1, 65)]


def confident(labels, rng, lo=120):
    C = rng.integers(lo, 256, (len(labels), 65))
    C[np.arange(len(labels)), labels] = rng.integers(0, 10, len(labels))
    return C.astype(np.uint8)


def edges(w):
    return sum((k + 1) * (k + 2) // 2 for k, _, _ in w)


def pack(words, tracks, gap=0):
    """words: lists of runs; tracks: lists of word indices; gap: slots of no track behind every track (they hold word 0)."""
    sp, rr, pr, first, n_of = R.pack([words])[:5]
    tf, members = [], []
    for t in tracks:
        tf.append(len(members))
        members += list(t) + [0] * gap
    return sp, rr, pr, first, n_of, np.array(tf, np.int32), np.array([len(t) for t in tracks], np.int32), np.array(members, np.int32)


def check(S, f, packed, B, dec=(0, 0), ins=64, dele=64, rounds=8, split=8, ref=True):
    """lattice_decode_tracks against lattice_decode_tracks_host and (ref) the reference; returns the records as tuples (DECODE_FIELDS),
    the labels, the member records as tuples (MEMBER_FIELDS), the sources and the parts."""
    f.set_bigram(B)
    f.set_word_decode(*dec)
    f.set_track_decode(ins, dele, rounds)
    f.set_run_split(1, 4, split)
    got = f.lattice_decode_tracks(*packed)
    host = S.lattice_decode_tracks_host(*packed, B, dec[0], dec[1], ins, dele, rounds, split)
    recs, hrecs = R.as_tuples(got[0]), R.as_tuples(host[0])
    assert recs == hrecs, [(g, a, b) for g, (a, b) in enumerate(zip(recs, hrecs)) if a != b][:5]
    mrec, hmrec = R.members_as_tuples(got[2]), R.members_as_tuples(host[2])
    assert mrec == hmrec, [(i, a, b) for i, (a, b) in enumerate(zip(mrec, hmrec)) if a != b][:5]
    for a, b in zip(got, host):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if ref:
        want = R.decode_tracks(*packed, B, dec[0], dec[1], ins, dele, rounds, split)
        assert recs == want[0], [(g, a, b) for g, (a, b) in enumerate(zip(recs, want[0])) if a != b][:5]
        assert (got[1] == want[1]).all() and mrec == want[2] and (got[3] == want[3]).all()
        assert [[int(p["run"]), int(p["piece"])] for p in got[4]] == want[4].tolist()
    return recs, got[1], mrec, got[3], got[4]


def test_the_recipe_under_every_setting(S, f):
    B, packed = make_case()
    for dec, rounds in (((0, 0), 0), ((0, 0), 1), ((0, 0), 64), ((64, 64), 8)):
        recs = check(S, f, packed, B, dec, 64, 64, rounds)[0]
        assert all(r[0] >= 0 for r in recs)
    assert any(r[3] >= 2 for r in recs) and any(r[3] == 0 and r[4] == 1 for r in recs)
    a = f.lattice_decode_tracks(*packed)
    b = f.lattice_decode_tracks(*packed)          # the same call twice: the same bytes
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_every_combination_of_cut_counts_under_every_setting(S, f):
    """Tracks of one member of one run and of two runs, the cut counts 0 .. 3 each, under the ends of every parameter."""
    rng = np.random.default_rng(81)
    B = rng.integers(0, 90, (66, 66)).astype(np.uint8)
    words = [word(rng, [k]) for k in range(4)] + [word(rng, [k, m]) for k in range(4) for m in range(4)]
    packed = pack(words, [[w] for w in range(len(words))])
    grid = itertools.product((1, 64, 255), (1, 64, 255), (0, 8, 255), (0, 1, 8, 64), ((0, 0), (64, 64)))
    for n, (ins, dele, split, rounds, dec) in enumerate(grid):
        recs, _, mrec, _, _ = check(S, f, packed, B, dec, ins, dele, rounds, split, ref=n % 9 == 0)
        assert all(r[5] == 1 for r in recs) and all(m[2] - m[3] + m[4] == r[2] for m, r in zip(mrec, recs))


def test_without_cuts_it_is_the_track_decode(S, f):
    rng = np.random.default_rng(82)
    B = rng.integers(0, 90, (66, 66)).astype(np.uint8)
    tracks = [TD.make_track(rng, [int(a) for a in rng.integers(0, 65, int(rng.integers(3, 9)))], int(rng.integers(1, 7))) for _ in range(6)]
    costs, first, n_of, tf, tc, members = TD.pack(tracks)
    packed = pack([plain(costs[int(a):int(a) + int(n)]) for a, n in zip(first, n_of)], [list(range(int(a), int(a) + int(n))) for a, n in zip(tf, tc)])
    for dec, rounds in (((0, 0), 8), ((64, 64), 2)):
        recs, ch, mrec, _, parts = check(S, f, packed, B, dec, 64, 64, rounds)
        plain_recs, pch, pmc = f.decode_tracks(costs, first, n_of, tf, tc, members)
        assert R.as_tuples(plain_recs) == recs and ch.tobytes() == pch.tobytes() and [m[0] for m in mrec] == pmc.tolist()
        assert [int(p["run"]) for p in parts] == list(range(len(costs))) and (parts["piece"] == -1).all()


def test_lengths_where_del_and_ins_switch_off(S, f):
    rng = np.random.default_rng(83)
    B = rng.integers(0, 40, (66, 66)).astype(np.uint8)
    T = [int(a) for a in rng.integers(0, 65, 32)]

    def touching(labels):
        """The labels as confident runs, the first two merged into a run of one cut whose pieces read them."""
        C = confident(labels, rng)
        if len(labels) < 2:
            return plain(C)
        return [run(1, rng.integers(150, 256, 65), [C[0], C[1]])] + plain(C[2:])
    words = [touching(T[:1]), touching(T[:1]), touching(T[:2])]                                 # 0 .. 2: l = 1 and 2
    words += [touching(T[:2]), touching(T[:2]), touching(T[:1])]                                # 3 .. 5
    words += [touching(T) for _ in range(3)] + [touching(T[:31])]                               # 6 .. 9: l = 32 and 31
    words += [touching(T[:31]) for _ in range(3)] + [touching(T)]                               # 10 .. 13
    tracks = [[0, 1], [2, 0, 1], [3, 4, 5], [6, 7, 8], [9, 6, 7, 8], [13, 10, 11, 12], [10, 11]]
    for rounds in (0, 8):
        recs, ch, mrec, _, _ = check(S, f, pack(words, tracks), B, (0, 0), 64, 64, rounds)
    assert [r[2] for r in recs] == [1, 1, 2, 32, 32, 31, 31]
    assert (ch[3] == T).all() and (ch[5, :31] == T[:31]).all()
    assert mrec[8][2:5] == (32, 0, 0)          # (the member reads its merged run as two pieces)


def test_node_counts_mixed_inside_a_track(S, f):
    rng = np.random.default_rng(84)
    B = rng.integers(0, 120, (66, 66)).astype(np.uint8)
    words = [[], word(rng, [3] * 8), word(rng, [3] * 8 + [0]), word(rng, [0] * 32), word(rng, [0] * 33), word(rng, [2, 0, 1]), word(rng, [1] * 16),
             plain(confident([3, 4, 5], rng))]
    assert [edges(w) for w in words[:3]] == [0, 80, 81]
    tracks = [list(range(8)), [7, 6, 5, 4, 3, 2, 1, 0], [0, 2, 7], [1, 7], [5, 6, 7, 7], [1], [0]]
    for dec in ((0, 0), (64, 64)):
        recs, _, mrec, src, _ = check(S, f, pack(words, tracks, gap=2), B, dec, 64, 64, 3)
        assert [r[5] for r in recs] == [6, 6, 2, 2, 4, 1, 1]
        assert mrec[2][0] == -1 and mrec[2][5] == 2 and mrec[4][0] == -1          # N = 33: unusable
        assert mrec[8][5] == -1 and mrec[9][5] == -1 and (src[8] == 255).all()    # slots of no track
        assert mrec[0][0] >= 0 and mrec[0][2] == 0 and mrec[0][4] == recs[0][2]   # N = 0: every label inserted


def test_special_tracks(S, f):
    rng = np.random.default_rng(85)
    B = rng.integers(0, 120, (66, 66)).astype(np.uint8)
    words = [word(rng, [1, 0, 2]), word(rng, [3] * 8 + [1]), word(rng, [0] * 40), word(rng, [2, 2]), []]
    tracks = [[], [0], [1, 2], [3, 3, 0], [4], [1, 0]]          # none, one, unusable only, a word twice, a word of no runs, unusable first
    recs, ch, mrec, _, _ = check(S, f, pack(words, tracks, gap=1), B)
    assert recs[0] == TD.NOT_DECODED and recs[2] == TD.NOT_DECODED and recs[4] == (-1, -1, 0, 0, 0, 1, -1, -1)
    assert (ch[0] == 255).all() and (ch[2] == 255).all() and recs[1][5:7] == (1, 0) and recs[3][5] == 3 and recs[5][5:7] == (1, 0)
    assert mrec[6][0] == mrec[7][0] >= 0 and mrec[3][0] == mrec[4][0] == -1
    dec = f.lattice_decode_words(*pack(words, tracks)[:5])[0]
    f.set_track_decode(64, 64, 0)
    one = f.lattice_decode_tracks(*pack(words, [[0], [3]]))[0]          # one usable member, the decoder's INS = DEL = 0
    assert int(one[0]["seed_cost"]) <= int(dec[0]["cost"]) and int(one[1]["seed_cost"]) <= int(dec[3]["cost"])
    none = f.lattice_decode_tracks(np.zeros(0, S.RUN_SPLIT_DTYPE), np.zeros((0, 65), np.uint8), np.zeros((0, 65), np.uint8), [], [], [], [], [])
    assert none[0].shape == (0,) and none[0].dtype == S.TRACK_DECODE_DTYPE and none[1].shape == (0, 32) and none[2].shape == (0,) and none[4].shape == (0,)
    check(S, f, pack(words, []), B)


def test_the_33rd_member_is_no_seed(S, f):
    B = np.full((66, 66), 10, np.uint8)
    A, Z = [5, 6, 7], [40, 41, 42]
    first32 = np.full((3, 65), 200, np.uint8)
    first32[np.arange(3), A] = 0
    first32[np.arange(3), Z] = 1
    last = np.full((3, 65), 255, np.uint8)
    last[np.arange(3), Z] = 0
    dear = np.full(65, 255, np.uint8)
    # the first two characters touch: a run of one cut that reads badly as a whole
    words = [[run(1, dear, [first32[0], first32[1]])] + plain(first32[2:])] * 32 + [[run(1, dear, [last[0], last[1]])] + plain(last[2:])]
    packed = pack(words, [list(range(33)), [32] + list(range(32))])
    recs, ch, _, _, _ = check(S, f, packed, B, rounds=0)
    assert list(ch[0, :3]) == A and recs[0][5] == 33 and 0 <= recs[0][6] < 32
    assert list(ch[1, :3]) == Z and recs[1][6] == 32          # Z wins where it is a seed
    recs, ch, mrec, _, _ = check(S, f, packed, B, rounds=8)
    assert list(ch[0, :3]) == Z and recs[0][3] == 3 and recs[0][4] == 1          # the polish finds it by three SUBs
    assert all(m[2:5] == (3, 0, 0) for m in mrec)


def test_lattice_decoder_strings_that_are_no_seeds(S, f):
    rng = np.random.default_rng(86)
    x = 64
    B = np.full((66, 66), 200, np.uint8)          # any two characters in a row are dear, but x between them is free: the decoder inserts
    B[:, x] = 0
    B[x, :] = 0
    B[65, :] = 0
    B[:, 65] = 0
    long_, short = confident(list(rng.integers(0, 60, 20)), rng), confident(list(rng.integers(0, 60, 10)), rng)
    words = [plain(long_), [], plain(np.full((3, 65), 255, np.uint8)), plain(short)]
    packed = pack(words, [[0, 1, 2, 3], [0, 1, 2], [3, 0]])
    dec, dch = S.lattice_decode_words_host(*packed[:5], B, 1, 200, 8)[:2]
    assert [int(d["n_chars"]) for d in dec] == [39, 0, 0, 19]          # more than 32, none (no runs), none (all dropped), a seed
    for rounds in (0, 2):
        recs, ch, mrec, _, _ = check(S, f, packed, B, (1, 200), 64, 64, rounds)
        assert recs[0][5:7] == (4, 3) and recs[1] == (-1, -1, 0, 0, 0, 3, -1, -1) and recs[2][5:7] == (2, 3)
        assert [m[0] for m in mrec[4:7]] == [-1, -1, -1]
    recs, ch, _, _, _ = check(S, f, packed, B, (1, 200), 64, 64, 0)
    assert (ch[0, :19] == dch[3, :19]).all() and recs[0][2] == 19


def test_both_sides_of_the_resident_rows_limit(S, f):
    """51 members of 10 edges and one of 2 or 3: 512 edges stay in LDS over the rounds, 513 are staged whenever they are read."""
    rng = np.random.default_rng(87)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    T = [7, 30, 52]

    def member():          # the three labels, the first two in a run of three cuts whose pieces (0, 2) and (2, 4) read them
        C = confident(T, rng, lo=40)
        pieces = [rng.integers(100, 256, 65) for _ in range(9)]
        pieces[1], pieces[7] = C[0], C[1]          # (the order of the pieces: (0,1) (0,2) (0,3) (1,2) (1,3) (1,4) (2,3) (2,4) (3,4))
        return [run(3, rng.integers(100, 256, 65), pieces), run(0, C[2], [])]
    words = [member() for _ in range(51)] + [word(rng, [0]), word(rng, [0, 0])]
    assert edges(words[0]) == 11
    words = [w[:1] for w in words[:51]] + words[51:]          # (one run of three cuts: 10 edges)
    below, above = list(range(51)) + [51, 51], list(range(51)) + [52, 51]
    assert sum(edges(words[w]) for w in below) == RES_EDGES and sum(edges(words[w]) for w in above) == RES_EDGES + 1
    for rounds in (0, 3):
        recs, ch, mrec, _, _ = check(S, f, pack(words, [below, above, above[::-1], below[:7]]), B, rounds=rounds, ref=False)
        assert [r[5] for r in recs] == [53, 53, 53, 7]
    assert list(ch[0, :2]) == T[:2] and mrec[0][2:5] == (2, 0, 0)
    check(S, f, pack(words, [above[:30] + [52] * 3, below[:9]]), B, rounds=2)          # ... and a smaller pair against the reference


def test_many_members(S, f):
    rng = np.random.default_rng(88)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    T = [7, 30, 52]
    words = []
    for _ in range(300):
        C = confident(T[:int(rng.integers(1, 4))], rng, lo=40)
        w = plain(C)
        if len(C) >= 2 and rng.random() < 0.5:
            w = [run(1, rng.integers(100, 256, 65), [C[0], C[1]])] + plain(C[2:])
        words.append(w)
    words.append(word(rng, [0] * 33))
    tracks = [list(range(300)), [300] + list(range(299, -1, -1)), list(range(0, 300, 7))]
    recs = check(S, f, pack(words, tracks), B, rounds=2, ref=False)[0]
    assert [r[5] for r in recs] == [300, 300, 43]
    # the member limit: 1024 one-atom members are decoded, 1025 are refused by both entry points and leave the context usable
    one = [plain(confident([9], rng, lo=40)) for _ in range(8)]
    recs, _, mrec, _, _ = check(S, f, pack(one, [[i % 8 for i in range(1024)]]), B, rounds=1, ref=False)
    assert recs[0][5] == 1024 and all(m[0] >= 0 for m in mrec)
    packed = pack(one, [[i % 8 for i in range(1025)]])
    for call in (lambda: f.lattice_decode_tracks(*packed), lambda: S.lattice_decode_tracks_host(*packed, B)):
        with pytest.raises(S.StrErError) as e:
            call()
        assert e.value.code == -7
    check(S, f, pack(one, [[0, 1, 2]]), B, rounds=1)


def test_only_the_index_and_the_first_candidate_decide(S, f):
    """Constant rows and rows of 255: every path of a member costs the same wherever SPLIT is 0, so edges of different spans into one node
    tie and only the order of the candidates decides the parts, only (J, index) the string."""
    for v in (7, 0, 255):
        const = lambda k: run(k, np.full(65, v), [np.full(65, v)] * LD.n_pieces(k))
        words = [[const(1), const(0)], [const(3)], [const(2), const(2)], [const(0), const(3), const(0)]]
        packed = pack(words, [[0, 1, 2], [1, 3], [2, 0], [3]])
        for B in (np.zeros((66, 66), np.uint8), np.full((66, 66), 255, np.uint8)):
            for ins, dele, split in ((64, 64, 0), (1, 1, 0), (255, 255, 8), (1, 1, 255), (7, 7, 0)):
                for rounds in (0, 1, 64):
                    check(S, f, packed, B, (0, 0), ins, dele, rounds, split, ref=rounds < 64 or ins == 7)


def test_65_tracks_in_one_call(S, f):
    rng = np.random.default_rng(89)
    B = rng.integers(0, 90, (66, 66)).astype(np.uint8)
    words = [word(rng, [int(k) for k in rng.integers(0, 4, int(rng.integers(1, 5)))], hi=200) for _ in range(65 * 5)]
    recs = check(S, f, pack(words, [list(range(5 * g, 5 * g + 5)) for g in range(65)]), B, rounds=4, ref=False)[0]
    assert len(recs) == 65 and all(r[5] == 5 for r in recs)


def test_no_table_and_bad_windows(S, f):
    rng = np.random.default_rng(90)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    words = [word(rng, [1, 0]), word(rng, [2])]
    packed = pack(words, [[0, 1]])
    f.set_bigram(None)
    with pytest.raises(S.StrErError) as e:
        f.lattice_decode_tracks(*packed)
    assert e.value.code == -6
    f.set_bigram(B)
    sp, rr, pr, first, n_of, tf, tc, mem = packed
    bad = [(sp, rr, pr, [0, 3], n_of, tf, tc, mem),                 # a word outside the runs
           (sp, rr, pr, first, n_of, tf, [3], mem),                 # a track outside the member array
           (sp, rr, pr, first, n_of, tf, tc, [0, 2]),               # a member outside the words
           (sp, rr, pr[:1], first, n_of, tf, tc, mem)]              # a run's pieces outside the piece rows
    for args in bad:
        for call in (lambda: f.lattice_decode_tracks(*args), lambda: S.lattice_decode_tracks_host(*args, B)):
            with pytest.raises(S.StrErError) as e:
                call()
            assert e.value.code == -1
    for v in (2, -1):
        assert f.L.str_er_set_lattice_track_decode(f.h, v) == -1
    recs = check(S, f, packed, B, rounds=8)[0]          # the context is usable after every refusal
    assert recs[0][5] == 2
