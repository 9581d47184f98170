"""The lattice decode pool on the GPU (str_er_track_pool_create_lattice_decode, _add_lattice, _join, _clear, _reset, _read_decode,
_read_lattice_decode, _lattice_members; the contract is at "The lattice decode pool" in str_er.h): every field of every record, every
label, member cost, member record, source byte and part of a read against the host entry point (str_er_lattice_decode_tracks_host) on
the kept list a numpy mirror computes (lattice_decode_pool_ref.py: keys, the `keep` newest, age order, rebased cells), with ==, at the
kernels' own edges: every combination of cut counts inside a member, the node counts 0, 1, 31, 32 and 33, tracks of no and of unusable
members, a word twice, a full cell (72 pieces, 80 edges) and one of 32 uncut runs, a piece table out of order with foreign pieces in
between, the rows decode pool on members without cuts, the age order at the seed limit, eviction inside one addition and across
additions, keep = 1, 32, 33 and 1024, kept lists on both sides of k_lattice_track_decode's LDS residency, joins in every grouping, the
member limit by counts alone, clear / reuse / reset, 300 slots in one call, a large pool read like a small one, the stale rules, the
refusals, and one pool reused by a larger and a smaller history."""
import numpy as np
import pytest

import lattice_decode_pool_ref as LP
import lattice_track_decode_ref as R
from test_lattice_track_decode import confident, edges, pack, plain, run, word

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def f(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    yield ctx
    ctx.close()


def setup(f, B, dec=(0, 0), ins=64, dele=64, rounds=8, split=8):
    f.set_bigram(B)
    f.set_word_decode(*dec)
    f.set_track_decode(ins, dele, rounds)
    f.set_run_split(1, 4, split)


def both(S, f, cap, keep):
    return S.LatticeDecodePool(f, cap, keep), LP.Mirror(cap, keep)


def add(pool, mirror, packed, slots):
    pool.add_lattice(*packed, slots)
    mirror.add(*packed, slots)


def nodes(w):
    return sum(k + 1 for k, _, _ in w)


def scattered(packed, rng):
    """The same call with the runs' pieces in another order in the piece table and foreign rows between them."""
    sp, rr, pr = packed[0].copy(), packed[1], packed[2]
    blocks, at = [], 0
    for r in rng.permutation(len(sp)):
        blocks.append(rng.integers(0, 256, (int(rng.integers(0, 3)), 65)).astype(np.uint8))          # foreign pieces
        at += len(blocks[-1])
        n = int(sp["n_pieces"][r])
        blocks.append(pr[int(sp["first_piece"][r]):int(sp["first_piece"][r]) + n])
        sp["first_piece"][r] = at
        at += n
    return (sp, rr, np.concatenate(blocks + [np.zeros((1, 65), np.uint8)])) + tuple(packed[3:])


def test_one_add_equals_the_one_call_decode(S, f):
    rng = np.random.default_rng(91)
    B = rng.integers(0, 90, (66, 66)).astype(np.uint8)
    # every combination of cut counts inside one member of two runs; N = 0, 1, 31, 32 and 33; a confident word
    combos = [word(rng, [k, m]) for k in range(4) for m in range(4)]
    sized = [[], word(rng, [0]), word(rng, [3] * 7 + [2]), word(rng, [3] * 8), word(rng, [3] * 8 + [0]), plain(confident([3, 4, 5], rng))]
    words = combos + sized
    assert [nodes(w) for w in sized] == [0, 1, 31, 32, 33, 3]
    n0 = len(combos)
    tracks = [list(range(n0)), [n0 + i for i in range(6)], [], [n0 + 4, n0 + 4], [n0 + 5, 3, n0 + 5, n0], [n0 + 4, n0 + 5], [n0]]
    packed = scattered(pack(words, tracks, gap=1), rng)
    n = len(tracks)
    for dec, split in (((0, 0), 8), ((64, 64), 8), ((0, 0), 0), ((64, 64), 0)):
        setup(f, B, dec, 64, 64, 3, split)
        pool, mirror = both(S, f, n + 1, 16)
        slots = list(range(n - 1, -1, -1))          # track g goes to slot n - 1 - g
        add(pool, mirror, packed, slots)
        rec, ch, mc, mrec, src, parts = LP.check_slots(S, pool, mirror, list(range(n + 1)), B, dec, 64, 64, 3, split)
        for s in range(n + 1):
            LP.check_members(pool, mirror, s)
        one = f.lattice_decode_tracks(*packed)
        host = S.lattice_decode_tracks_host(*packed, B, dec[0], dec[1], 64, 64, 3, split)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(one, host))
        tf = packed[5]
        for g, t in enumerate(tracks):
            i, usable = slots[g], [j for j, w in enumerate(t) if nodes(words[w]) <= 32]
            r, o = rec[i], one[0][g]
            assert [int(r[k]) for k in LP.FIELDS[:6]] + [int(r["lm_cost"])] == [int(o[k]) for k in LP.FIELDS[:6]] + [int(o["lm_cost"])]
            assert int(r["n_members"]) == len(t) and int(r["n_kept"]) == len(usable) == int(r["n_used"])
            assert (int(r["seed_member"]) < 0 and int(o["seed_member"]) < 0) or t[usable[int(r["seed_member"])]] == int(o["seed_member"])
            assert ch[i].tobytes() == one[1][g].tobytes()
            om = one[2][[int(tf[g]) + j for j in usable]]
            for k in ("cost", "n_parts", "n_del", "n_ins"):
                assert mrec[i][:len(usable)][k].tolist() == om[k].tolist()
            assert mrec[i][:len(usable)]["word"].tolist() == list(range(len(usable)))
            assert src[i][:len(usable)].tobytes() == one[3][[int(tf[g]) + j for j in usable]].tobytes()
        assert LP.as_tuples(rec)[n] == LP.EMPTY and (ch[n] == 255).all() and (mc[n] == -1).all()          # a slot never named
        pool.close()


def test_cell_edges(S, f):
    rng = np.random.default_rng(92)
    B = rng.integers(0, 90, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=2)
    full, wide, small = word(rng, [3] * 8), word(rng, [0] * 32), word(rng, [1, 0, 2])
    assert edges(full) == 80 and nodes(full) == 32 and sum(len(p) for _, _, p in full) == 72 and nodes(wide) == 32
    words = [full, wide, small]
    pool, mirror = both(S, f, 4, 4)
    add(pool, mirror, scattered(pack(words, [[0], [1], [2, 0, 1, 2]]), rng), [0, 1, 2])
    add(pool, mirror, scattered(pack(words, [[1, 0]]), rng), [0])          # ... and mixed in a slot
    _, _, _, mrec, _, parts = LP.check_slots(S, pool, mirror, [0, 1, 2, 3], B, rounds=2)
    for s in range(4):
        LP.check_members(pool, mirror, s)
    assert int(parts["piece"].max()) >= 80 and (parts["piece"] < 80 * 4).all() and (parts["run"] < 32 * 4).all()
    pool.close()


def test_without_cuts_it_is_the_decode_pool(S, f):
    rng = np.random.default_rng(93)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    rows = [confident(list(rng.integers(0, 65, int(m))), rng) for m in (3, 4, 2, 5, 3, 1, 0)] + [rng.integers(0, 256, (33, 65)).astype(np.uint8)]
    from test_track_decode import pack as pack_rows
    for dec, rounds in (((0, 0), 2), ((64, 64), 8)):
        setup(f, B, dec, 64, 64, rounds)
        pool, mirror = both(S, f, 3, 3)
        rows_pool = S.DecodePool(f, 3, 3)
        for tracks, slots in (([[0, 1], [2]], [0, 1]), ([[3, 7, 4], [5, 6]], [1, 2]), ([[7], [0, 0, 1, 2]], [0, 1])):
            add(pool, mirror, pack([plain(r) for r in rows], tracks), slots)
            rows_pool.add(*pack_rows(rows, tracks), slots)
        pool.join(0, [2]); mirror.join(0, [2]); rows_pool.join(0, [2])
        got = LP.check_slots(S, pool, mirror, [0, 1, 2], B, dec, 64, 64, rounds)
        want = rows_pool.read([0, 1, 2])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], want))
        assert (got[5]["piece"] == -1).all()
        k, n, rr = rows_pool.members(1)
        k2, n2, _, rr2, _ = pool.members(1)
        assert k.tolist() == k2.tolist() and n.tolist() == n2.tolist() and all(rr[i][:n[i]].tobytes() == rr2[i][:n[i]].tobytes() for i in range(len(k)))
        pool.close(); rows_pool.close()


def test_age_order_eviction_and_the_seed_limit(S, f):
    B = np.full((66, 66), 10, np.uint8)
    A, Z = [5, 6, 7], [40, 41, 42]
    first32 = np.full((3, 65), 200, np.uint8)
    first32[np.arange(3), A] = 0
    first32[np.arange(3), Z] = 1
    last = np.full((3, 65), 255, np.uint8)
    last[np.arange(3), Z] = 0
    # (the first two runs of `last` touch: a run of one cut whose pieces read them)
    touching = [run(1, np.full(65, 255), [last[0], last[1]]), run(0, last[2], [])]
    words = [plain(first32)] * 32 + [touching]
    setup(f, B, rounds=0)
    pool, mirror = both(S, f, 4, 40)
    orders = [list(range(33)), [32] + list(range(32))]
    for slot, order in enumerate(orders):
        for w in order:
            add(pool, mirror, pack(words, [[w]]), [slot])
    rec, ch = LP.check_slots(S, pool, mirror, [0, 1], B, rounds=0)[:2]
    assert ch[0, :3].tolist() == A and ch[1, :3].tolist() == Z and int(rec[1]["seed_member"]) == 0 and rec["n_kept"].tolist() == [33, 33]
    # the age order is not the order of the cells: the oldest member arrives last, by a join
    add(pool, mirror, pack(words, [[32]]), [3])
    for w in range(32):
        add(pool, mirror, pack(words, [[w]]), [2])
    pool.join(2, [3]); mirror.join(2, [3])
    rec, ch = LP.check_slots(S, pool, mirror, [2, 3], B, rounds=0)[:2]
    assert ch[0, :3].tolist() == Z and int(rec[0]["seed_member"]) == 0 and rec["n_kept"].tolist() == [33, 0]
    pool.close()
    # eviction inside one addition and across additions, keep = 1, 32, 33
    rng = np.random.default_rng(94)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=1)
    words = [word(rng, [int(k) for k in rng.integers(0, 4, int(m))]) for m in (1, 2, 3, 2, 1, 3)] + [word(rng, [3] * 9)]
    for keep in (1, 32, 33):
        pool, mirror = both(S, f, 2, keep)
        for t in ([0, 1, 6, 2], [int(w) for w in rng.integers(0, 7, 40)], [3], [4, 6, 5]):
            add(pool, mirror, pack(words, [t], gap=1), [1])
            LP.check_slots(S, pool, mirror, [0, 1], B, rounds=1)
            keys = LP.check_members(pool, mirror, 1)
            assert len(keys) <= keep and keys == sorted(keys)
        assert keys[-1] == 4 << 32 | 2 and len(keys) == min(keep, len(mirror.kept[1]))
        pool.close()


def test_both_sides_of_the_resident_rows(S, f):
    rng = np.random.default_rng(95)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=2)
    six, wide, one = word(rng, [1, 1, 0]), word(rng, [3, 3, 1, 0, 0]), word(rng, [0])          # 7, 25 and 1 edges
    assert (edges(six), edges(wide), edges(one)) == (7, 25, 1)
    words = [six, wide, one]
    pool, mirror = both(S, f, 2, 40)
    # 20 x 25 + 12 = 512 edges, and the same with one more
    add(pool, mirror, pack(words, [[1] * 20 + [0] + [2] * 5, [1] * 20 + [0] + [2] * 6]), [0, 1])
    assert [sum(edges(words[w]) for w in t) for t in ([1] * 20 + [0] + [2] * 5, [1] * 20 + [0] + [2] * 6)] == [512, 513]
    rec = LP.check_slots(S, pool, mirror, [0, 1], B, rounds=2)[0]
    assert rec["n_kept"].tolist() == [26, 27] and (rec["cost"] >= 0).all()
    pool.close()


def test_join_is_a_merge_in_every_grouping(S, f):
    rng = np.random.default_rng(96)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=2)
    words = [word(rng, [int(k) for k in rng.integers(0, 4, int(m))]) for m in (2, 3, 1, 2, 3, 1)]
    history = [([0, 1], 0), ([2], 1), ([3, 4], 2), ([5, 0], 1), ([1], 2), ([2, 3], 0), ([4, 5], 2)]
    reads = []
    for joins in ([(0, [1, 2])], [(0, [1]), (0, [2])], [(0, [2]), (0, [1])], [(1, [2]), (0, [1])]):
        pool, mirror = both(S, f, 4, 3)
        for t, slot in history:
            add(pool, mirror, scattered(pack(words, [t]), rng), [slot])
        for dst, srcs in joins:
            pool.join(dst, srcs); mirror.join(dst, srcs)
            LP.check_slots(S, pool, mirror, [0, 1, 2, 3], B, rounds=2)
        keys = LP.check_members(pool, mirror, 0)
        assert keys == [6 << 32 | 1, 7 << 32 | 0, 7 << 32 | 1]
        rec = pool.read([0, 1, 2])[0]
        assert LP.as_tuples(rec)[0][8:] == (12, 3) and LP.as_tuples(rec)[1] == LP.as_tuples(rec)[2] == LP.EMPTY          # the srcs read empty
        reads.append(LP.snapshot(pool, [0, 1, 2]))
        pool.join(0, [])                                       # no srcs
        pool.join(3, [0]); mirror.join(3, [0])                 # an empty dst
        LP.check_slots(S, pool, mirror, [3, 0], B, rounds=2)
        LP.check_members(pool, mirror, 3)
        add(pool, mirror, pack(words, [[0], [1]]), [0, 3])      # ... and the slots go on
        LP.check_slots(S, pool, mirror, [0, 3], B, rounds=2)
        pool.close()
    assert reads[0] == reads[1] == reads[2] == reads[3]


def test_the_member_limit_clear_reuse_and_reset(S, f):
    rng = np.random.default_rng(97)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=1)
    words = [word(rng, [1]), word(rng, [0, 2])]
    pool, mirror = both(S, f, 3, 1)
    add(pool, mirror, pack(words, [[0] * 40000, [1] * 25536]), [0, 1])
    add(pool, mirror, pack(words, [[1]]), [2])
    before = LP.snapshot(pool, [0, 1, 2])
    assert pool.read([0, 1, 2])[0]["n_members"].tolist() == [40000, 25536, 1] and pool.members(0)[0].tolist() == [1 << 32 | 39999]
    for call in (lambda: pool.join(0, [1, 2]), lambda: pool.add_lattice(*pack(words, [[0] * 25537]), [0]), lambda: pool.add_lattice(*pack(words, [[0] * 40001]), [1])):
        with pytest.raises(S.StrErError) as e:
            call()
        assert e.value.code == -7 and LP.snapshot(pool, [0, 1, 2]) == before
    pool.join(0, [1]); mirror.join(0, [1])                     # 65536 exactly
    rec = LP.check_slots(S, pool, mirror, [0, 1, 2], B, rounds=1)[0]
    assert rec["n_members"].tolist() == [65536, 0, 1] and pool.members(0)[0].tolist() == [1 << 32 | 65535]
    add(pool, mirror, pack(words, [[0]]), [1])                  # the refused additions took no serial
    assert pool.members(1)[0].tolist() == [3 << 32]
    pool.close()
    pool, mirror = both(S, f, 3, 2)
    keys = []
    for _ in range(2):
        add(pool, mirror, pack(words, [[0, 1, 0], [1]]), [0, 2])
        pool.clear([0, 0]); mirror.clear([0])
        rec = LP.check_slots(S, pool, mirror, [0, 1, 2], B, rounds=1)[0]
        assert LP.as_tuples(rec)[0] == LP.EMPTY and pool.members(0)[0].tolist() == [] and pool.info()["in_use"] == 1
        add(pool, mirror, pack(words, [[1], [1, 0]]), [0, 1])          # a cleared slot takes new members
        LP.check_slots(S, pool, mirror, [0, 1, 2], B, rounds=1)
        keys.append([LP.check_members(pool, mirror, s) for s in range(3)])
        pool.reset(); mirror.reset()
        assert LP.as_tuples(LP.check_slots(S, pool, mirror, [0, 1, 2], B, rounds=1)[0]) == [LP.EMPTY] * 3
    assert keys[0] == keys[1] == [[2 << 32], [2 << 32 | 1, 2 << 32 | 2], [1 << 32 | 3]]          # after reset the serial restarts
    info = pool.info()
    assert info["decode"] and info["lattice"] and info["n_entries"] == 0 and info["keep"] == 2 and info["cap_tracks"] == 3 and not info["stale"]
    assert info["device_bytes"] >= 3 * 2 * 9072
    pool.close()


def test_scale_in_one_call(S, f):
    rng = np.random.default_rng(98)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=1)
    words = [word(rng, [int(k) for k in rng.integers(0, 3, int(rng.integers(1, 3)))], hi=200) for _ in range(24)] + [word(rng, [3] * 9)]
    tracks = [[int(w) for w in rng.integers(0, 25, int(k))] for k in rng.integers(0, 5, 300)]
    packed, order = pack(words, tracks), [int(s) for s in rng.permutation(300)]
    pool, mirror = both(S, f, 300, 2)
    add(pool, mirror, packed, order)
    rec = LP.check_slots(S, pool, mirror, list(range(0, 300, 7)) + [299, 0, 0, 150], B, rounds=1)[0]
    got = pool.read_lattice(list(range(300)))
    assert int(got[0]["n_kept"].max()) == 2 and int(got[0]["n_kept"].min()) == 0 and int((got[0]["n_members"] > 2).sum()) > 50
    # three slots of a 4096-slot pool read as the same slots of a small pool with the same history
    big = S.LatticeDecodePool(f, 4096, 2)
    big.add_lattice(*packed, order)
    pick = [order[3], order[200], 299]
    assert LP.snapshot(big, pick) == LP.snapshot(pool, pick)
    big.close(); pool.close()
    # one slot of keep = 1024 with 1030 small members
    small = [word(rng, [int(k)]) for k in (0, 1, 0, 2, 0, 0, 1, 0)]
    pool, mirror = both(S, f, 1, 1024)
    at = 0
    for n in (500, 500, 30):
        add(pool, mirror, pack(small, [[(at + i) % 8 for i in range(n)]]), [0])
        at += n
    rec, _, mc = LP.check_slots(S, pool, mirror, [0], B, rounds=1)[:3]
    keys = LP.check_members(pool, mirror, 0)
    assert LP.as_tuples(rec)[0][8:] == (1030, 1024) and int(rec[0]["n_used"]) == 1024 and (mc >= 0).all()
    assert keys[0] == 1 << 32 | 6 and keys[-1] == 3 << 32 | 29
    pool.close()


def test_stale_rules(S, f):
    rng = np.random.default_rng(99)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=2)
    f.set_lexicon(["AB", "CDE", "F1"], fold_case=False)
    words = [word(rng, [1, 0]), word(rng, [0, 0, 2])]
    packed = pack(words, [[0, 1], [1]])
    from test_track_decode import pack as pack_rows
    rows_packed = pack_rows([confident([10, 11], rng), confident([12, 13, 14], rng)], [[0, 1], [1]])
    pool, mirror = both(S, f, 2, 2)
    rows_pool, lex = S.DecodePool(f, 2, 2), S.TrackPool(f, 2)
    lex.add(*rows_packed, [0, 1])
    rows_pool.add(*rows_packed, [0, 1])
    lex_before = lex.read([0, 1]).tobytes()
    add(pool, mirror, packed, [1, 0])
    try:
        # the decode side's setters: both decode pools are stale until reset, the lexicon pool is not touched
        for setter, args in ((f.set_bigram, (B,)), (f.set_word_decode, (0, 0)), (f.set_track_decode, (64, 64, 2))):
            setter(*args)
            assert pool.info()["stale"] and rows_pool.info()["stale"] and not lex.info()["stale"] and lex.read([0, 1]).tobytes() == lex_before
            for call in (lambda: pool.read([0]), lambda: pool.read_lattice([0]), lambda: pool.add_lattice(*packed, [0, 1]), lambda: pool.join(0, [1]),
                         lambda: pool.clear([0]), lambda: pool.members(0)):
                with pytest.raises(S.StrErError) as e:
                    call()
                assert e.value.code == -6
            pool.reset(); mirror.reset(); rows_pool.reset()
            rows_pool.add(*rows_packed, [0, 1])
            assert not pool.info()["stale"] and LP.as_tuples(pool.read([0, 1])[0]) == [LP.EMPTY] * 2
            add(pool, mirror, packed, [1, 0])
            LP.check_slots(S, pool, mirror, [0, 1], B, rounds=2)
        # SPLIT is compared by value: another num / den or the same SPLIT again leave the pool usable; another SPLIT makes it stale and the
        # old one makes it usable again, with the same bytes.  The rows decode pool never goes stale on set_run_split, the lexicon pool does.
        before, rows_before = LP.snapshot(pool, [0, 1]), rows_pool.read([0, 1])
        for args, stale in (((1, 4, 8), False), ((1, 3, 8), False), ((1, 4, 9), True), ((1, 4, 8), False)):
            f.set_run_split(*args)
            assert pool.info()["stale"] == stale and not rows_pool.info()["stale"] and lex.info()["stale"]
            assert all(a.tobytes() == b.tobytes() for a, b in zip(rows_before, rows_pool.read([0, 1])))
            if stale:
                with pytest.raises(S.StrErError) as e:
                    pool.read_lattice([0])
                assert e.value.code == -6
            else:
                assert LP.snapshot(pool, [0, 1]) == before
            lex.reset()
        # _reset rebinds: under the new SPLIT the pool reads as the host does with it
        f.set_run_split(1, 4, 40)
        assert pool.info()["stale"]
        pool.reset(); mirror.reset()
        add(pool, mirror, packed, [0, 1])
        LP.check_slots(S, pool, mirror, [0, 1], B, rounds=2, split=40)
        # the lexicon side's other setters do not touch it
        before = LP.snapshot(pool, [0, 1])
        for setter, args in ((f.set_lexicon, (["AB", "CDE", "F1"], False)), (f.set_word_match, (64, 64, 2))):
            setter(*args)
            assert lex.info()["stale"] and not pool.info()["stale"] and LP.snapshot(pool, [0, 1]) == before
            lex.reset()
    finally:
        lex.close(); rows_pool.close(); pool.close()
        f.set_lexicon([])
        f.set_run_split(1, 4, 8)


def test_the_error_matrix(S, f):
    rng = np.random.default_rng(100)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=2)
    f.set_lexicon(["AB", "CDE"], fold_case=False)
    words = [word(rng, [1, 0]), word(rng, [2])]
    packed = pack(words, [[0, 1], [1]])
    from test_track_decode import pack as pack_rows
    rows_packed = pack_rows([confident([10, 11], rng)], [[0]])
    pool, mirror = both(S, f, 3, 2)
    add(pool, mirror, packed, [0, 1])
    before = LP.snapshot(pool, [0, 1, 2])
    rows_pool, lex, lat = S.DecodePool(f, 2, 2), S.TrackPool(f, 2), S.TrackPool(f, 2, lattice=True)
    L, C = f.L, __import__("ctypes")
    sl = np.array([0, 1], np.int32)
    n, buf = C.c_int32(), np.zeros(1 << 16, np.uint8)
    ptr = lambda a: a.ctypes.data
    try:
        # the kinds: what each entry point answers on which pool
        def code(fn):
            with pytest.raises(S.StrErError) as e:
                fn()
            return e.value.code
        assert code(lambda: S.TrackPool.add(pool, *rows_packed, [0])) == -6
        assert code(lambda: S.TrackPool.read(pool, [0])) == -6
        assert code(lambda: S.DecodePool.members(pool, 0)) == -6
        assert code(lambda: S.TrackPool.add_lattice(rows_pool, *packed, [0, 1])) == -6
        for other in (rows_pool, lex, lat):
            assert L.str_er_track_pool_read_lattice_decode(other.h, ptr(sl), 1, ptr(buf), ptr(buf), ptr(buf), None, None, None, 0, C.byref(n)) == -6
            assert L.str_er_track_pool_lattice_members(other.h, 0, None, None, None, None, None, C.byref(n)) == -6
        for flags in (2, 3):
            h = C.c_void_p()
            assert L.str_er_track_pool_create(f.h, 2, flags, C.byref(h)) == -1 and not h.value
        h = C.c_void_p()
        assert L.str_er_track_pool_create_lattice_decode(f.h, 0, 2, C.byref(h)) == -1 and L.str_er_track_pool_create_lattice_decode(f.h, 2, 1025, C.byref(h)) == -1
        assert L.str_er_track_pool_create_lattice_decode(f.h, 2, 0, C.byref(h)) == -1 and L.str_er_track_pool_create_lattice_decode(f.h, 13108, 1024, C.byref(h)) == -7
        assert LP.snapshot(pool, [0, 1, 2]) == before
        # the arguments: a slot named twice, out of range, a piece outside the rows, a member outside the words, cap_parts too small
        bad_piece = (packed[0].copy(),) + tuple(packed[1:])
        bad_piece[0]["first_piece"][0] = len(packed[2])
        bad_member = tuple(packed[:7]) + (np.array([0, 1, 2], np.int32),)
        for call, want in ((lambda: pool.add_lattice(*packed, [1, 1]), -1), (lambda: pool.add_lattice(*packed, [0, 3]), -1), (lambda: pool.add_lattice(*packed, [0, -1]), -1),
                           (lambda: pool.add_lattice(*bad_piece, [0, 1]), -1), (lambda: pool.add_lattice(*bad_member, [0, 1]), -1), (lambda: pool.read_lattice([3]), -1),
                           (lambda: pool.read([-1]), -1), (lambda: pool.members(3), -1), (lambda: pool.join(0, [0]), -1), (lambda: pool.join(0, [1, 1]), -1),
                           (lambda: pool.clear([3]), -1), (lambda: pool.add(*rows_packed, [0]), -6)):
            assert code(call) == want
            assert LP.snapshot(pool, [0, 1, 2]) == before
        total = len(pool.read_lattice([0, 1])[5])
        out, ch, mc = np.zeros(2, S.POOL_DECODE_DTYPE), np.zeros((2, 32), np.uint8), np.zeros((2, 2), np.int32)
        parts = np.zeros(total, S.SPLIT_PART_DTYPE)
        assert total >= 2
        assert L.str_er_track_pool_read_lattice_decode(pool.h, ptr(sl), 2, ptr(out), ptr(ch), ptr(mc), None, None, ptr(parts), total - 1, C.byref(n)) == -7 and n.value == total
        assert not out.tobytes().strip(b"\0") and not parts.tobytes().strip(b"\0")          # nothing was written
        assert L.str_er_track_pool_read_lattice_decode(pool.h, ptr(sl), 2, ptr(out), ptr(ch), ptr(mc), None, None, ptr(parts), total, C.byref(n)) == 0 and n.value == total
        assert parts.tobytes() == pool.read_lattice([0, 1])[5].tobytes()
        # members_out, src and parts may be NULL, each on its own
        assert L.str_er_track_pool_read_lattice_decode(pool.h, ptr(sl), 2, ptr(out), ptr(ch), ptr(mc), None, None, None, 0, C.byref(n)) == 0 and n.value == total
        assert LP.snapshot(pool, [0, 1, 2]) == before
        LP.check_slots(S, pool, mirror, [0, 1, 2], B, rounds=2)
    finally:
        for p in (rows_pool, lex, lat, pool):
            p.close()
        f.set_lexicon([])


def test_one_pool_reused_by_a_larger_and_a_smaller_history(S, f):
    rng = np.random.default_rng(101)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=2)
    cases = {}
    for size, n_tracks in (("small", 3), ("large", 48)):
        r = np.random.default_rng(7)
        tracks = [R.make_track(r, [int(a) for a in r.integers(0, 65, int(r.integers(2, 7)))], int(r.integers(1, 5))) for _ in range(n_tracks)]
        cases[size] = (R.pack(tracks), n_tracks)
    pool, mirror = both(S, f, 64, 6)
    rounds = []
    for size in ("small", "large", "small"):
        packed, n = cases[size]
        slots = list(range(n))
        add(pool, mirror, packed, slots)
        add(pool, mirror, scattered(packed, np.random.default_rng(3)), slots[::-1])          # every track again, into another slot
        pool.join(0, [n - 1]); mirror.join(0, [n - 1])
        LP.check_slots(S, pool, mirror, slots + [63], B, rounds=2)
        for s in slots[:4]:
            LP.check_members(pool, mirror, s)
        rounds.append(LP.snapshot(pool, slots[:3] + [63]))
        pool.reset(); mirror.reset()
    assert rounds[0] == rounds[2] != rounds[1]
    pool.close()
