"""The track pool on the GPU (str_er_track_pool_*; the contract is at str_er_pool_match): every record read from a slot against the host
entry points (str_er_match_tracks_host, in lattice mode str_er_lattice_match_tracks_host) on the concatenation of everything the slot
was given, with ==, on the made-up rows of test_track_read.py and test_lattice_track.py at the kernels' own edges -- the buckets of the
run count mixed in a track, an addition that widens the lengths tried, the order and the grouping of the additions, a chunk of 16 groups
of the lexicon with padding slots that would win if they counted, joins and clears, 300 slots in one call, the member limit, the errors
and the stale pool, and the lattice mode."""
import itertools

import numpy as np
import pytest

import lattice_match_ref as LM
import word_match_ref as WM
from test_lattice_decode_abi import cheapen, make_rows
from test_lattice_track import SETTINGS, _spans, _words

pytestmark = pytest.mark.gpu
EMPTY = (-1, -1, -1, -1, 0, 0, 0, 0)
SEVEN = ("entry", "cost", "second_entry", "second_cost", "free_cost", "n_tried", "n_used")


@pytest.fixture(scope="module")
def f(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    yield ctx
    ctx.close()


def setup(S, f, words, fold, ins, dele, band, split, cap, lattice=False):
    f.set_lexicon(words, fold_case=fold)
    f.set_word_match(ins, dele, band)
    f.set_run_split(1, 4, split)
    return S.TrackPool(f, cap, lattice=lattice)


def flat(lists):
    tc = np.array([len(t) for t in lists], np.int32)
    tf = (np.concatenate([[0], np.cumsum(tc)[:-1]]) if len(lists) else np.zeros(0)).astype(np.int32)
    return tf, tc, np.array([w for t in lists for w in t], np.int32)


def as_pool(S, rec, counts):
    out = np.zeros(len(rec), S.POOL_MATCH_DTYPE)
    for k in SEVEN:
        out[k] = rec[k]
    out["n_members"] = counts
    return out


def reference(S, rows, lists, words, setting):
    """The records of the slots that were given the member lists `lists`.  rows: (costs, first, n_of) or (splits, run rows, piece rows,
    first, n_of)."""
    fold, ins, dele, band, split = setting
    tf, tc, mem = flat(lists)
    if len(rows) == 3:
        rec = S.match_tracks_host(*rows, tf, tc, mem, words, fold, ins, dele, band)[0]
    else:
        rec = S.lattice_match_tracks_host(*rows, tf, tc, mem, words, fold, ins, dele, band, split)[0]
    return as_pool(S, rec, tc)


def check(S, pool, slots, rows, lists, words, setting):
    got, want = pool.read(slots), reference(S, rows, lists, words, setting)
    assert got.dtype == S.POOL_MATCH_DTYPE and got.tolist() == want.tolist(), [(s, tuple(a), tuple(b)) for s, a, b in zip(slots, got, want) if a != b][:5]
    assert got.tobytes() == pool.read(slots).tobytes()
    return got


@pytest.mark.parametrize("setting", SETTINGS)
def test_one_add_equals_the_track_match(S, f, setting):
    """Run counts 8 / 9, 16 / 17 and 32 / 33 mixed in a track, a track of unusable members and a track of none."""
    fold, ins, dele, band, split = setting
    rng = np.random.default_rng(7000 + ins)
    first, n_of = _spans([8, 9, 16, 17, 32, 33, 40, 1, 0, 5])
    costs = cheapen(rng, rng.integers(0, 256, (int(n_of.sum()), 65)).astype(np.uint8))
    words = _words(rng, 300, 1, 12) + _words(rng, 60, 14, 20, labels=8) + _words(rng, 40, 28, 32, labels=8)
    lists = [[0, 1], [2, 3], [4, 5], [0, 3, 4, 9], [5, 6], [], [7], [8], [9, 9, 1]]
    pool = setup(S, f, words, fold, ins, dele, band, split, len(lists) + 1)
    try:
        tf, tc, mem = flat(lists)
        slots = list(range(len(lists)))[::-1]
        pool.add(costs, first, n_of, tf, tc, mem, slots)
        got = check(S, pool, slots, (costs, first, n_of), lists, words, setting)
        rec, _ = f.match_tracks(costs, first, n_of, tf, tc, mem)
        assert [tuple(r)[:7] for r in got.tolist()] == [tuple(r)[:7] for r in rec.tolist()]
        assert tuple(got[4])[:4] == (-1, -1, -1, -1) and got[4]["free_cost"] > 0 and tuple(got[4])[5:] == (0, 0, 2)          # unusable members alone
        assert tuple(got[5]) == EMPTY and tuple(pool.read([len(lists)])[0]) == EMPTY                                      # a track of none; a slot never named
        info = pool.info()
        assert info["cap_tracks"] == len(lists) + 1 and not info["lattice"] and info["n_entries"] == len(words) and info["in_use"] == len(lists) - 1 and not info["stale"]
        assert info["device_bytes"] >= (len(lists) + 1) * 4 * 64
    finally:
        pool.close()


def test_an_add_that_widens_the_lengths_tried(S, f):
    """Band 0: a member of 3 runs, a read, then a member of 7 runs.  The entries of length 7 must carry the first member's distance:
    an accumulation that skips the lengths outside the adding member's band gives another record, which is computed here as well."""
    setting = (False, 64, 64, 0, 8)
    rng = np.random.default_rng(7100)
    first, n_of = _spans([3, 7])
    costs = cheapen(rng, rng.integers(0, 256, (10, 65)).astype(np.uint8))
    words = _words(rng, 40, 3, 3, labels=10) + _words(rng, 40, 7, 7, labels=10) + _words(rng, 20, 5, 5, labels=10)
    pool = setup(S, f, words, *setting, 2)
    try:
        pool.add(costs, first, n_of, [0], [1], [0], [1])
        one = check(S, pool, [1], (costs, first, n_of), [[0]], words, setting)
        assert one[0]["n_tried"] == 40
        pool.add(costs, first, n_of, [0], [1], [1], [1])
        two = check(S, pool, [1], (costs, first, n_of), [[0, 1]], words, setting)
        assert two[0]["n_tried"] == 80 and two[0]["n_members"] == 2
        lex, keys = WM.Lexicon(words, False), []
        for l, (ix, E) in lex.by_len.items():
            if l not in (3, 7):
                continue
            C = costs[:3] if l == 3 else costs[3:]          # only the member whose band holds l
            keys += list(zip(WM.entry_costs(C.astype(np.int64), E, 64, 64).tolist(), ix.tolist()))
        skipped = min(keys)
        assert (skipped[1], skipped[0]) != (int(two[0]["entry"]), int(two[0]["cost"])) and skipped[0] < int(two[0]["cost"])
    finally:
        pool.close()


@pytest.mark.parametrize("lattice", [False, True])
def test_the_grouping_and_the_order_of_the_additions_change_no_byte(S, f, lattice):
    setting = SETTINGS[0]
    rng = np.random.default_rng(7200)
    first, n_of = _spans([2, 5, 9, 1, 12, 3, 33, 7])
    sp, rc, pc = make_rows(S, rng, rng.integers(0, 3, int(n_of.sum())) if lattice else np.zeros(int(n_of.sum()), np.int64))
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    words = _words(rng, 200, 1, 14, labels=12)
    rows = (sp, rc, pc, first, n_of) if lattice else (rc, first, n_of)
    pool = setup(S, f, words, *setting, 8, lattice)
    try:
        add = pool.add_lattice if lattice else pool.add
        for slot, (order, calls) in enumerate(itertools.product((list(range(8)), list(range(8))[::-1]), (1, 2, 4, 8))):
            for part in np.array_split(np.array(order), calls):
                add(*rows, [0], [len(part)], part, [slot])
        got = check(S, pool, list(range(8)), rows, [list(range(8))] * 8, words, setting)
        assert all(got[k].tobytes() == got[0].tobytes() for k in range(8)) and got[0]["n_used"] == 7 and got[0]["n_members"] == 8
    finally:
        pool.close()


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_one_length_around_a_chunk_of_16_groups(S, f, n):
    """n entries of 5 characters without the label 0, on rows where the label 0 is free: the padding slots of the last group (all
    label 0) would beat every entry if they counted.  The runner-up sits in the last slot -- for n > 1024 in another chunk."""
    setting = (False, 64, 64, 2, 8)
    rng = np.random.default_rng(7300 + n)
    costs = rng.integers(60, 256, (5, 65)).astype(np.uint8)
    costs[:, 0] = 0
    E = rng.integers(1, 65, (n, 5))
    E[3] = [11, 22, 33, 44, 55]
    E[n - 1] = [11, 22, 33, 44, 56]
    costs[np.arange(5), E[3]] = 1
    costs[4, 56] = 2
    words = ["".join(WM.ALPHABET[a] for a in e) for e in E]
    pool = setup(S, f, words, *setting, 2)
    try:
        pool.add(costs, [0], [5], [0], [2], [0, 0], [1])
        got = check(S, pool, [1, 0], (costs, [0], [5]), [[0, 0], []], words, setting)
        assert tuple(got[0])[:4] == (3, 10, n - 1, 12) and got[0]["n_tried"] == n and tuple(got[1]) == EMPTY
    finally:
        pool.close()


def test_a_lexicon_of_the_lengths_1_and_32_only(S, f):
    setting = (True, 40, 90, 1, 8)
    rng = np.random.default_rng(7400)
    first, n_of = _spans([1, 32, 31, 2, 16])
    costs = cheapen(rng, rng.integers(0, 256, (int(n_of.sum()), 65)).astype(np.uint8))
    words = _words(rng, 70, 1, 1) + _words(rng, 70, 32, 32, labels=8)
    pool = setup(S, f, words, *setting, 4)
    try:
        lists = [[0, 3], [1, 2], [4], [4, 0, 1]]          # the length 1 alone, 32 alone, neither (nothing tried), both
        pool.add(costs, first, n_of, *flat(lists), [0, 1, 2, 3])
        got = check(S, pool, [0, 1, 2, 3], (costs, first, n_of), lists, words, setting)
        assert got["n_tried"].tolist() == [70, 70, 0, 140] and got[2]["entry"] == -1 and got[2]["n_used"] == 1
    finally:
        pool.close()


@pytest.mark.parametrize("lattice", [False, True])
def test_join_and_clear(S, f, lattice):
    setting = SETTINGS[1]
    rng = np.random.default_rng(7500)
    first, n_of = _spans([2, 4, 6, 9, 3, 1])
    sp, rc, pc = make_rows(S, rng, rng.integers(0, 4, int(n_of.sum())) if lattice else np.zeros(int(n_of.sum()), np.int64))
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    words = _words(rng, 150, 1, 10, labels=12)
    rows = (sp, rc, pc, first, n_of) if lattice else (rc, first, n_of)
    pool = setup(S, f, words, *setting, 6, lattice)
    try:
        add = pool.add_lattice if lattice else pool.add
        lists = [[0, 1], [2], [3, 4, 5], [], [5, 5], [1]]
        add(*rows, *flat(lists), list(range(6)))
        pool.join(0, [1])                                      # two slots
        lists[0], lists[1] = lists[0] + lists[1], []
        check(S, pool, list(range(6)), rows, lists, words, setting)
        pool.join(3, [2, 4])                                   # three, into an empty one
        lists[3], lists[2], lists[4] = lists[2] + lists[4], [], []
        pool.join(5, [1])                                      # a used one and an empty one; and no source at all
        pool.join(5, [])
        got = check(S, pool, list(range(6)), rows, lists, words, setting)
        assert [tuple(got[s]) for s in (1, 2, 4)] == [EMPTY] * 3 and pool.info()["in_use"] == 3
        pool.clear([0, 0, 3])                                  # a slot named twice
        lists[0], lists[3] = [], []
        add(*rows, [0], [2], [4, 2], [3])                      # the cleared slot again: nothing stale
        lists[3] = [4, 2]
        check(S, pool, list(range(6)), rows, lists, words, setting)
        for dst, srcs in ((0, [0]), (0, [1, 1]), (6, [0]), (0, [6]), (-1, [0])):
            with pytest.raises(S.StrErError) as e:
                pool.join(dst, srcs)
            assert e.value.code == -1
        check(S, pool, list(range(6)), rows, lists, words, setting)
    finally:
        pool.close()


def test_300_tracks_into_300_slots_in_descending_order(S, f):
    setting = SETTINGS[0]
    rng = np.random.default_rng(7600)
    first, n_of = _spans(rng.integers(0, 7, 40))
    costs = cheapen(rng, rng.integers(0, 256, (int(n_of.sum()), 65)).astype(np.uint8))
    words = _words(rng, 90, 1, 8, labels=12)
    lists = [[int(w) for w in rng.integers(0, 40, int(k))] for k in rng.integers(0, 4, 300)]
    pool = setup(S, f, words, *setting, 300)
    try:
        slots = list(range(300))[::-1]
        pool.add(costs, first, n_of, *flat(lists), slots)
        check(S, pool, slots, (costs, first, n_of), lists, words, setting)
        assert pool.info()["in_use"] == sum(1 for t in lists if t)
    finally:
        pool.close()


def test_the_member_limit(S, f):
    """65536 copies of a word of one run in one slot in one call against 64 entries; one more is refused and the record stays."""
    setting = (False, 255, 255, 31, 8)
    costs = np.full((1, 65), 255, np.uint8)
    words = ["".join(WM.ALPHABET[(k + t) % 65] for t in range(32)) for k in range(64)]
    pool = setup(S, f, words, *setting, 2)
    try:
        mem = np.zeros(65536, np.int32)
        pool.add(costs, [0], [1], [0], [65536], mem, [1])
        got = check(S, pool, [1], (costs, [0], [1]), [mem.tolist()], words, setting)
        assert tuple(got[0]) == (0, 65536 * 32 * 255, 1, 65536 * 32 * 255, 65536 * 255, 64, 65536, 65536)
        for slots in ([1], [0, 1]):                            # alone, and behind a track that would fit
            with pytest.raises(S.StrErError) as e:
                pool.add(costs, [0], [1], list(range(len(slots))), [1] * len(slots), [0] * len(slots), slots)
            assert e.value.code == -7
        pool.add(costs, [0], [1], [0], [1], [0], [0])
        with pytest.raises(S.StrErError) as e:
            pool.join(0, [1])
        assert e.value.code == -7
        assert pool.read([1]).tobytes() == got.tobytes() and pool.read([0])[0]["n_members"] == 1
    finally:
        pool.close()


def test_errors_and_the_stale_pool(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    try:
        rng = np.random.default_rng(7700)
        with pytest.raises(S.StrErError) as e:                # no lexicon
            S.TrackPool(ctx, 4)
        assert e.value.code == -6 and "lexicon" in str(e.value)
        words = _words(rng, 50, 2, 9)
        ctx.set_lexicon(words)
        for cap in (0, -1):
            with pytest.raises(S.StrErError) as e:
                S.TrackPool(ctx, cap)
            assert e.value.code == -1
        setting = (True, 64, 64, 2, 8)
        first, n_of = _spans([3, 2])
        sp, rc, pc = make_rows(S, rng, np.array([1, 0, 3, 0, 2]))
        pool, lat = S.TrackPool(ctx, 4), S.TrackPool(ctx, 4, lattice=True)
        try:
            pool.add(rc, first, n_of, [0], [2], [0, 1], [2])
            lat.add_lattice(sp, rc, pc, first, n_of, [0], [2], [0, 1], [2])
            want, lwant = pool.read([2]), lat.read([2])
            bad = [dict(slots=[0, 0], tf=[0, 1], tc=[1, 1]), dict(slots=[4]), dict(slots=[-1]), dict(mem=[0, 2]), dict(tf=[1], tc=[2]), dict(first=[3, 0])]
            for kw in bad:                                     # a slot twice, out of range; a member outside the words, a track outside the members, a word outside the rows
                a = dict(first=first, tf=[0], tc=[2], mem=[0, 1], slots=[1])
                a.update(kw)
                for call in (lambda: pool.add(rc, a["first"], n_of, a["tf"], a["tc"], a["mem"], a["slots"]),
                             lambda: lat.add_lattice(sp, rc, pc, a["first"], n_of, a["tf"], a["tc"], a["mem"], a["slots"])):
                    with pytest.raises(S.StrErError) as e:
                        call()
                    assert e.value.code == -1, kw
            with pytest.raises(S.StrErError) as e:            # the wrong mode, both ways
                pool.add_lattice(sp, rc, pc, first, n_of, [0], [2], [0, 1], [1])
            assert e.value.code == -6
            with pytest.raises(S.StrErError) as e:
                lat.add(rc, first, n_of, [0], [2], [0, 1], [1])
            assert e.value.code == -6
            for slots in ([4], [-1]):
                for call in (pool.read, pool.clear):
                    with pytest.raises(S.StrErError) as e:
                        call(slots)
                    assert e.value.code == -1
            assert len(pool.read([])) == 0
            assert pool.read([2]).tobytes() == want.tobytes() and lat.read([2]).tobytes() == lwant.tobytes() and pool.info()["in_use"] == 1
            assert want.tolist() == reference(S, (rc, first, n_of), [[0, 1]], words, setting).tolist()
            assert lwant.tolist() == reference(S, (sp, rc, pc, first, n_of), [[0, 1]], words, setting).tolist()
            # the setters make both pools stale until reset; the context works all the while
            for setter, now in ((lambda: ctx.set_word_match(3, 200, 1), (True, 3, 200, 1, 8)), (lambda: ctx.set_run_split(1, 4, 0), (True, 3, 200, 1, 0)),
                                (lambda: ctx.set_lexicon(words[:30] + _words(rng, 2000, 1, 6), fold_case=False), None)):
                setter()
                for p in (pool, lat):
                    assert p.info()["stale"]
                    for call in (lambda: p.read([2]), lambda: p.clear([2]), lambda: p.join(0, [1]), lambda: p.add(rc, first, n_of, [0], [2], [0, 1], [1]),
                                 lambda: p.add_lattice(sp, rc, pc, first, n_of, [0], [2], [0, 1], [1])):
                        with pytest.raises(S.StrErError) as e:
                            call()
                        assert e.value.code == -6
                assert len(ctx.match_tracks(rc, first, n_of, [0], [2], [0, 1])[0]) == 1
                pool.reset(); lat.reset()
                assert not pool.info()["stale"] and pool.info()["in_use"] == 0 and tuple(pool.read([2])[0]) == EMPTY
                lex = words if now else ctx._lexicon
                now = now or (False, 3, 200, 1, 0)
                pool.add(rc, first, n_of, [0], [2], [0, 1], [2])
                lat.add_lattice(sp, rc, pc, first, n_of, [0], [2], [0, 1], [2])
                assert pool.read([2]).tolist() == reference(S, (rc, first, n_of), [[0, 1]], lex, now).tolist()
                assert lat.read([2]).tolist() == reference(S, (sp, rc, pc, first, n_of), [[0, 1]], lex, now).tolist()
            assert pool.info()["n_entries"] == 2030
            ctx.set_lexicon([])
            with pytest.raises(S.StrErError) as e:            # a reset without a lexicon: still stale
                pool.reset()
            assert e.value.code == -6 and pool.info()["stale"]
        finally:
            pool.close(); lat.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("setting", SETTINGS)
def test_lattice_tracks_of_one_for_every_combination_of_cut_counts(S, f, setting):
    fold, ins, dele, band, split = setting
    rng = np.random.default_rng(7800 + ins + band)
    combos = [c for R in (1, 2, 3) for c in itertools.product(range(4), repeat=R)]          # 84 words, each a track of one
    first, n_of = _spans([len(c) for c in combos])
    sp, rc, pc = make_rows(S, rng, np.array([k for c in combos for k in c]))
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    words = _words(rng, 150, 1, 9, labels=12) + _words(rng, 10, 10, 14, labels=12)
    nw = len(combos)
    pool = setup(S, f, words, *setting, nw, lattice=True)
    try:
        pool.add_lattice(sp, rc, pc, first, n_of, np.arange(nw), np.ones(nw, np.int32), np.arange(nw), np.arange(nw))
        got = check(S, pool, np.arange(nw), (sp, rc, pc, first, n_of), [[w] for w in range(nw)], words, setting)
        one = f.lattice_match_words(sp, rc, pc, first, n_of)[0]
        assert [tuple(r)[:6] for r in got.tolist()] == [r[:6] for r in LM.as_tuples(one)]
    finally:
        pool.close()


def test_lattice_mixed_members_and_the_uncut_pool(S, f):
    """Cut and uncut members, the buckets 8 / 16 / 32 and an unusable member in one slot, added in two calls; and on uncut runs a lattice
    pool holds the bytes of a pool of rows."""
    setting = (True, 40, 50, 2, 8)
    rng = np.random.default_rng(7900)
    shapes = [[0, 0, 0], [1, 2], [3, 3], [3] * 8, [3] * 8 + [0], [3] * 4, [0] * 33, [0] * 32, [2, 1] * 3 + [0, 1], []]
    first, n_of = _spans([len(c) for c in shapes])
    sp, rc, pc = make_rows(S, rng, np.array([k for c in shapes for k in c], np.int64))
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    words = _words(rng, 40, 1, 1) + _words(rng, 40, 32, 32, labels=6) + _words(rng, 200, 2, 31, labels=6)
    rows = (sp, rc, pc, first, n_of)
    pool = setup(S, f, words, *setting, 4, lattice=True)
    try:
        lists = [[0, 1, 2, 3, 4, 5], [4, 6], [], [3, 7]]
        pool.add_lattice(*rows, *flat(lists), [0, 1, 2, 3])
        check(S, pool, [0, 1, 2, 3], rows, lists, words, setting)
        more = [[8, 9, 1], [6], [7, 0], []]
        pool.add_lattice(*rows, *flat(more), [0, 1, 2, 3])
        got = check(S, pool, [0, 1, 2, 3], rows, [a + b for a, b in zip(lists, more)], words, setting)
        assert got[0]["n_used"] == 8 and got[0]["n_members"] == 9 and tuple(got[1])[:4] == (-1, -1, -1, -1) and got[1]["free_cost"] > 0
    finally:
        pool.close()
    first, n_of = _spans([8, 9, 16, 17, 32, 33, 1, 2, 0, 5])
    sp, rc, pc = make_rows(S, rng, np.zeros(int(n_of.sum()), np.int64))
    rc = cheapen(rng, rc)
    lists = [[0], [1, 2], [3, 4, 5], [9, 8], [3, 0, 4, 1, 5, 2, 6, 7]]
    lat = setup(S, f, words, *setting, 5, lattice=True)
    plain = S.TrackPool(f, 5)
    try:
        lat.add_lattice(sp, rc, pc, first, n_of, *flat(lists), range(5))
        plain.add(rc, first, n_of, *flat(lists), range(5))
        assert lat.read(range(5)).tobytes() == plain.read(range(5)).tobytes()
        check(S, plain, range(5), (rc, first, n_of), lists, words, setting)
    finally:
        lat.close(); plain.close()
