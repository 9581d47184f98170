"""The decode pool on the GPU (str_er_track_pool_create_decode, _add, _join, _clear, _reset, _read_decode, _members; the contract is at
str_er_pool_decode): every field of every record, every label and every member cost of a read against the host entry point
(str_er_decode_tracks_host) on the kept list a numpy mirror computes (decode_pool_ref.py: keys, the `keep` newest, age order), with ==,
at the kernels' own edges: the row counts 0 .. 40 mixed inside a track, tracks of no and of unusable members, the age order at the seed
limit, eviction inside one addition and across additions, keep = 1, 32, 33 and 1024, kept lists on both sides of k_track_decode's LDS
residency, joins in every grouping, the member limit by counts alone, clear / reuse / reset, 300 slots in one call, the stale rules in
both directions and one context reused by a larger and a smaller history."""
import numpy as np
import pytest

import decode_pool_ref as DP
import read_chain_cases as RC
from test_track_decode import confident, pack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def f(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    yield ctx
    ctx.close()


def setup(f, B, dec=(0, 0), ins=64, dele=64, rounds=8):
    f.set_bigram(B)
    f.set_word_decode(*dec)
    f.set_track_decode(ins, dele, rounds)


def both(S, f, cap, keep):
    return S.DecodePool(f, cap, keep), DP.Mirror(cap, keep)


def add(pool, mirror, packed, slots):
    pool.add(*packed, slots)
    mirror.add(*packed, slots)


def single(words, order):
    """One addition per word of `order`, each a track of that one member."""
    return [pack(words, [[w]]) for w in order]


def test_one_add_equals_the_one_call_decode(S, f):
    for seed, gap, dec, rounds in ((32, 2, (0, 0), 3), (32, 2, (64, 64), 3), (33, 1, (0, 0), 8)):
        rng = np.random.default_rng(seed)
        B = rng.integers(0, 120, (66, 66)).astype(np.uint8)
        if seed == 32:          # the words and tracks of test_row_counts_mixed_inside_a_track
            words = [rng.integers(0, 256, (m, 65)).astype(np.uint8) for m in (0, 1, 8, 9, 16, 17, 32, 33)] + [confident([3, 4, 5], rng)]
            tracks = [list(range(8)), [7, 6, 5, 4, 3, 2, 1, 0], [0, 7, 8], [6, 8], [1, 2, 8, 8]]
        else:                   # ... and of test_special_tracks: none, one, unusable only, a word twice, a word of no rows, unusable first
            words = [confident([1, 2, 3], rng), rng.integers(0, 256, (33, 65)).astype(np.uint8), rng.integers(0, 256, (40, 65)).astype(np.uint8),
                     confident([1, 9, 3, 4], rng), np.zeros((0, 65), np.uint8)]
            tracks = [[], [0], [1, 2], [3, 3, 0], [4], [1, 0]]
        packed = pack(words, tracks, gap=gap)
        setup(f, B, dec, 64, 64, rounds)
        n = len(tracks)
        pool, mirror = both(S, f, n + 1, 8)
        slots = list(range(n - 1, -1, -1))          # track g goes to slot n - 1 - g
        add(pool, mirror, packed, slots)
        rec, ch, mc = DP.check_slots(S, pool, mirror, list(range(n + 1)), B, dec, 64, 64, rounds)
        one, och, omc = f.decode_tracks(*packed)
        host, hch, hmc = S.decode_tracks_host(*packed, B, dec[0], dec[1], 64, 64, rounds)
        assert one.tobytes() == host.tobytes() and och.tobytes() == hch.tobytes() and omc.tobytes() == hmc.tobytes()
        n_of, tf, mem = packed[2], packed[3], packed[5]
        for g, t in enumerate(tracks):
            r, usable = rec[slots[g]], [j for j, w in enumerate(t) if n_of[w] <= 32]
            assert [int(r[k]) for k in DP.FIELDS[:6]] + [int(r["lm_cost"])] == [int(one[g][k]) for k in DP.FIELDS[:6]] + [int(one[g]["lm_cost"])]
            assert int(r["n_members"]) == len(t) and int(r["n_kept"]) == len(usable) == int(r["n_used"])
            assert (int(r["seed_member"]) < 0 and int(one[g]["seed_member"]) < 0) or t[usable[int(r["seed_member"])]] == int(one[g]["seed_member"])
            assert ch[slots[g]].tolist() == och[g].tolist()
            assert mc[slots[g]][:len(usable)].tolist() == [int(omc[tf[g] + j]) for j in usable] and (mc[slots[g]][len(usable):] == -1).all()
        assert DP.as_tuples(rec)[n] == DP.EMPTY and (ch[n] == 255).all() and (mc[n] == -1).all()          # a slot never named
        pool.close()


def test_age_order_is_observable(S, f):
    B = np.full((66, 66), 10, np.uint8)
    A, Z = [5, 6, 7], [40, 41, 42]
    first32 = np.full((3, 65), 200, np.uint8)
    first32[np.arange(3), A] = 0
    first32[np.arange(3), Z] = 1
    last = np.full((3, 65), 255, np.uint8)
    last[np.arange(3), Z] = 0
    words = [first32] * 32 + [last]
    orders = [list(range(33)), [32] + list(range(32))]
    # on the host alone: the 33rd member is no seed, so the two orders of the same members give different strings
    for order, want in zip(orders, (A, Z)):
        _, ch, _ = S.decode_tracks_host(*pack([words[w] for w in order], [list(range(33))]), B, 0, 0, 64, 64, 0)
        assert ch[0, :3].tolist() == want
    setup(f, B, rounds=0)
    pool, mirror = both(S, f, 4, 40)
    for slot, order in enumerate(orders):
        for p in single(words, order):
            add(pool, mirror, p, [slot])
    rec, ch, _ = DP.check_slots(S, pool, mirror, [0, 1], B, rounds=0)
    assert ch[0, :3].tolist() == A and ch[1, :3].tolist() == Z and int(rec[1]["seed_member"]) == 0 and rec["n_kept"].tolist() == [33, 33]
    # the second order again where the age order is not the order of the cells: the oldest member arrives last, by a join
    for slot, order in ((3, [32]), (2, list(range(32)))):
        for p in single(words, order):
            add(pool, mirror, p, [slot])
    pool.join(2, [3])
    mirror.join(2, [3])
    rec, ch, _ = DP.check_slots(S, pool, mirror, [2, 3], B, rounds=0)
    assert ch[0, :3].tolist() == Z and int(rec[0]["seed_member"]) == 0 and rec["n_kept"].tolist() == [33, 0]
    pool.close()


def test_eviction(S, f):
    rng = np.random.default_rng(41)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=2)
    words = [confident(list(rng.integers(0, 65, int(m))), rng) for m in (3, 4, 2, 5, 3, 1)] + [rng.integers(0, 256, (33, 65)).astype(np.uint8)]
    # keep = 3: additions of 2, 2 and 1 members; every state is read
    pool, mirror = both(S, f, 2, 3)
    for t in ([0, 1], [2, 3], [4]):
        add(pool, mirror, pack(words, [t]), [1])
        DP.check_slots(S, pool, mirror, [0, 1], B, rounds=2)
        keys = DP.check_members(pool, mirror, 1)
    assert keys.tolist() == [2 << 32 | 0, 2 << 32 | 1, 3 << 32 | 0] and pool.read([1])[0]["n_members"].tolist() == [5]
    pool.close()
    # keep = 2: one addition [u, x, u, u, x, u], x unusable: the newest two usable by position stay
    pool, mirror = both(S, f, 1, 2)
    add(pool, mirror, pack(words, [[0, 6, 1, 2, 6, 3]]), [0])
    rec, _, _ = DP.check_slots(S, pool, mirror, [0], B, rounds=2)
    keys, n_runs, _ = pool.members(0)
    DP.check_members(pool, mirror, 0)
    assert keys.tolist() == [1 << 32 | 3, 1 << 32 | 5] and n_runs.tolist() == [2, 5] and DP.as_tuples(rec)[0][8:] == (6, 2)
    pool.close()
    # keep = 1
    pool, mirror = both(S, f, 2, 1)
    for t in ([0, 1, 6], [6], [2], [3, 6]):
        add(pool, mirror, pack(words, [t, [4]]), [0, 1])
        DP.check_slots(S, pool, mirror, [1, 0], B, rounds=2)
        DP.check_members(pool, mirror, 0)
    assert pool.members(0)[0].tolist() == [4 << 32 | 0] and pool.members(1)[0].tolist() == [4 << 32 | 2]
    pool.close()


@pytest.mark.parametrize("keep", [32, 33])
def test_keep_at_the_seed_limit(S, f, keep):
    rng = np.random.default_rng(42)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=1)
    T = [7, 30, 52, 11]
    words = [confident(T[:int(rng.integers(1, 5))], rng, lo=40) for _ in range(34)]
    pool, mirror = both(S, f, 2, keep)
    for lo, hi in ((0, 20), (20, 21), (21, 34)):          # 34 members in three additions
        add(pool, mirror, pack(words, [list(range(lo, hi))]), [1])
    rec, _, _ = DP.check_slots(S, pool, mirror, [1, 0], B, rounds=1)
    DP.check_members(pool, mirror, 1)
    assert DP.as_tuples(rec)[0][8:] == (34, keep) and DP.as_tuples(rec)[1] == DP.EMPTY
    pool.close()


def test_kept_lists_at_the_residency_edge_of_the_track_decode(S, f):
    B = RC.bigram()
    setup(f, B, rounds=8)
    case = RC.track_decode_case("large")
    packed = case["packed"]
    rows = [sum(case["rows_of"][w] for w in t) for t in case["tracks"][:3]]
    assert rows == [288, 252, 253]          # nine members of 32 rows; 7 x 32 + 28, the last list that stays in LDS; one row more
    pool, mirror = both(S, f, 3, 9)
    add(pool, mirror, packed[:3] + (packed[3][:3], packed[4][:3], packed[5]), [2, 0, 1])
    rec, _, _ = DP.check_slots(S, pool, mirror, [0, 1, 2], B, rounds=8)
    assert rec["n_kept"].tolist() == [8, 8, 9] and (rec["cost"] >= 0).all()
    pool.close()


def test_join_is_a_merge_not_a_concatenation(S, f):
    rng = np.random.default_rng(43)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=2)
    words = [confident(list(rng.integers(0, 65, int(m))), rng) for m in (3, 4, 2, 5, 3, 1, 4, 2)]
    history = (([0, 1], 0), ([2, 3], 1), ([4, 5], 0), ([6, 7], 2))          # serials 1 .. 4: slot 0 holds older and newer members than slot 1
    reads = []
    for joins in (((0, [1, 2]),), ((0, [1]), (0, [2])), ((0, [2]), (0, [1]))):
        pool, mirror = both(S, f, 4, 3)
        for t, slot in history:
            add(pool, mirror, pack(words, [t]), [slot])
        for dst, srcs in joins:
            pool.join(dst, srcs)
            mirror.join(dst, srcs)
            DP.check_slots(S, pool, mirror, [0, 1, 2, 3], B, rounds=2)
        keys = DP.check_members(pool, mirror, 0)
        assert keys.tolist() == [3 << 32 | 1, 4 << 32 | 0, 4 << 32 | 1]
        rec, ch, mc = pool.read([0, 1, 2])
        assert DP.as_tuples(rec)[0][8:] == (8, 3) and DP.as_tuples(rec)[1] == DP.as_tuples(rec)[2] == DP.EMPTY          # the srcs read empty
        reads.append(rec.tobytes() + ch.tobytes() + mc.tobytes() + pool.members(0)[2][:, :1].tobytes())
        pool.join(0, [])                                       # no srcs
        pool.join(3, [0])                                      # an empty dst
        mirror.join(3, [0])
        DP.check_slots(S, pool, mirror, [3, 0], B, rounds=2)
        DP.check_members(pool, mirror, 3)
        add(pool, mirror, pack(words, [[0], [1]]), [0, 3])      # ... and the slots go on
        DP.check_slots(S, pool, mirror, [0, 3], B, rounds=2)
        pool.close()
    assert reads[0] == reads[1] == reads[2]


def test_the_member_limit_by_counts_alone(S, f):
    rng = np.random.default_rng(44)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=1)
    words = [confident([9], rng, lo=40), confident([12], rng, lo=40)]
    pool, mirror = both(S, f, 3, 1)
    add(pool, mirror, pack(words, [[0] * 40000, [1] * 25536]), [0, 1])
    add(pool, mirror, pack(words, [[1]]), [2])
    before = DP.check_slots(S, pool, mirror, [0, 1, 2], B, rounds=1)
    assert before[0]["n_members"].tolist() == [40000, 25536, 1] and pool.members(0)[0].tolist() == [1 << 32 | 39999]
    for call in (lambda: pool.join(0, [1, 2]), lambda: pool.add(*pack(words, [[0] * 25537]), [0]), lambda: pool.add(*pack(words, [[0] * 40001]), [1])):
        with pytest.raises(S.StrErError) as e:
            call()
        assert e.value.code == -7
        after = pool.read([0, 1, 2])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    pool.join(0, [1])                                          # 65536 exactly
    mirror.join(0, [1])
    rec, _, _ = DP.check_slots(S, pool, mirror, [0, 1, 2], B, rounds=1)
    assert rec["n_members"].tolist() == [65536, 0, 1] and pool.members(0)[0].tolist() == [1 << 32 | 65535]
    add(pool, mirror, pack(words, [[0]]), [1])                  # the refused additions took no serial
    assert pool.members(1)[0].tolist() == [3 << 32]
    pool.close()


def test_clear_reuse_and_reset(S, f):
    rng = np.random.default_rng(45)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=2)
    words = [confident(list(rng.integers(0, 65, int(m))), rng) for m in (3, 4, 2, 5)]
    pool, mirror = both(S, f, 3, 2)
    keys = []
    for _ in range(2):
        add(pool, mirror, pack(words, [[0, 1, 2], [3]]), [0, 2])
        pool.clear([0, 0])
        mirror.clear([0])
        rec, _, _ = DP.check_slots(S, pool, mirror, [0, 1, 2], B, rounds=2)
        assert DP.as_tuples(rec)[0] == DP.EMPTY and pool.members(0)[0].tolist() == [] and pool.info()["in_use"] == 1
        add(pool, mirror, pack(words, [[3], [1, 0]]), [0, 1])          # a cleared slot takes new members
        DP.check_slots(S, pool, mirror, [0, 1, 2], B, rounds=2)
        keys.append([DP.check_members(pool, mirror, s).tolist() for s in range(3)])
        pool.reset()
        mirror.reset()
        rec, _, _ = DP.check_slots(S, pool, mirror, [0, 1, 2], B, rounds=2)
        assert DP.as_tuples(rec) == [DP.EMPTY] * 3
    assert keys[0] == keys[1] == [[2 << 32], [2 << 32 | 1, 2 << 32 | 2], [1 << 32 | 3]]          # after reset the serial restarts
    info = pool.info()
    assert info["decode"] and not info["lattice"] and info["n_entries"] == 0 and info["keep"] == 2 and info["cap_tracks"] == 3 and not info["stale"]
    pool.close()


def test_300_slots_in_one_add_and_one_read(S, f):
    rng = np.random.default_rng(46)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=2)
    T = [7, 30, 52]
    words = [confident(T[:int(rng.integers(1, 4))], rng, lo=40) for _ in range(40)] + [rng.integers(0, 256, (33, 65)).astype(np.uint8)]
    tracks = [[int(w) for w in rng.integers(0, 41, int(k))] for k in rng.integers(0, 5, 300)]
    pool, mirror = both(S, f, 300, 2)
    add(pool, mirror, pack(words, tracks), [int(s) for s in rng.permutation(300)])
    rec, _, _ = DP.check_slots(S, pool, mirror, list(range(300)) + [299, 0, 0, 150], B, rounds=2)
    assert int(rec["n_kept"].max()) == 2 and int(rec["n_kept"].min()) == 0 and int((rec["n_members"] > 2).sum()) > 50
    pool.close()


def test_keep_1024(S, f):
    rng = np.random.default_rng(36)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=1)
    one = [confident([9], rng, lo=40) for _ in range(8)]
    pool, mirror = both(S, f, 1, 1024)
    at = 0
    for n in (500, 500, 30):          # 1030 one-row members
        add(pool, mirror, pack(one, [[(at + i) % 8 for i in range(n)]]), [0])
        at += n
    rec, _, mc = DP.check_slots(S, pool, mirror, [0], B, rounds=1)
    keys = DP.check_members(pool, mirror, 0)
    assert DP.as_tuples(rec)[0][8:] == (1030, 1024) and int(rec[0]["n_used"]) == 1024 and (mc >= 0).all()
    assert int(keys[0]) == 1 << 32 | 6 and int(keys[-1]) == 3 << 32 | 29
    pool.close()


def test_stale_rules_in_both_directions(S, f):
    rng = np.random.default_rng(47)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    setup(f, B, rounds=2)
    f.set_lexicon(["AB", "CDE", "F1"], fold_case=False)
    words = [confident([10, 11], rng), confident([12, 13, 14], rng)]
    packed = pack(words, [[0, 1], [1]])
    pool, mirror = both(S, f, 2, 2)
    lex = S.TrackPool(f, 2)
    lex.add(*packed, [0, 1])
    lex_before = lex.read([0, 1]).tobytes()
    add(pool, mirror, packed, [1, 0])
    try:
        # the decode side's setters: the decode pool is stale until reset, the lexicon pool is not touched
        for setter, args in ((f.set_bigram, (B,)), (f.set_word_decode, (0, 0)), (f.set_track_decode, (64, 64, 2))):
            setter(*args)
            assert pool.info()["stale"] and not lex.info()["stale"] and lex.read([0, 1]).tobytes() == lex_before
            for call in (lambda: pool.read([0]), lambda: pool.add(*packed, [0, 1]), lambda: pool.join(0, [1]), lambda: pool.clear([0]), lambda: pool.members(0)):
                with pytest.raises(S.StrErError) as e:
                    call()
                assert e.value.code == -6
            pool.reset()
            mirror.reset()
            assert not pool.info()["stale"] and DP.as_tuples(pool.read([0, 1])[0]) == [DP.EMPTY] * 2
            add(pool, mirror, packed, [1, 0])
            DP.check_slots(S, pool, mirror, [0, 1], B, rounds=2)
        # the lexicon side's setters: the lexicon pool is stale, the decode pool goes on with the same bytes
        before = pool.read([0, 1])
        for setter, args in ((f.set_lexicon, (["AB", "CDE", "F1"], False)), (f.set_word_match, (64, 64, 2)), (f.set_run_split, (1, 4, 8))):
            setter(*args)
            assert lex.info()["stale"] and not pool.info()["stale"]
            assert all(a.tobytes() == b.tobytes() for a, b in zip(before, pool.read([0, 1])))
            lex.reset()
        add(pool, mirror, packed, [0, 1])
        DP.check_slots(S, pool, mirror, [0, 1], B, rounds=2)
    finally:
        lex.close()
        pool.close()
        f.set_lexicon([])


def test_one_context_reused_by_a_larger_and_a_smaller_history(S, f):
    B = RC.bigram()
    setup(f, B, rounds=2)
    cases = {size: RC.track_decode_case(size) for size in RC.SIZES}
    assert len(cases["large"]["packed"][5]) >= 16 * len(cases["small"]["packed"][5])
    pool, mirror = both(S, f, 64, 12)
    rounds = []
    for size in ("small", "large", "small"):
        packed, n = cases[size]["packed"], len(cases[size]["tracks"])
        slots = list(range(n))
        add(pool, mirror, packed, slots)
        add(pool, mirror, packed, slots[::-1])                           # every track again, into another slot
        pool.join(0, [n - 1])
        mirror.join(0, [n - 1])
        rec, ch, mc = DP.check_slots(S, pool, mirror, slots + [63], B, rounds=2)
        rounds.append(rec.tobytes() + ch.tobytes() + mc.tobytes() + b"".join(DP.check_members(pool, mirror, s).tobytes() for s in slots))
        pool.reset()
        mirror.reset()
    assert rounds[0] == rounds[2] != rounds[1]
    pool.close()
