"""The lexicon kernels on lexicons past one pass of their merges (big_lexicon_cases.py; the scenarios are proven on the layout mirror
and the references in test_lexicon_layout.py): 1024, 1025 and 2049 groups on the track side (64, 65 and 129 chunks of 16 groups: the
last full single pass of the lane-strided merges, a second and a third pass), 4097 groups on the word side (65 chunks of 64 groups) and
2^20 entries (1024 and 256 chunks) under a band of 1.  Every scenario runs against every kernel family it applies to -- match_tracks,
lattice_match_tracks and the track pool in both modes on the track side, match_words and lattice_match_words on the word side -- and
every record field, member cost, source byte and part is compared with == against the numpy reference and byte for byte against the
host entry point; the pool against the host entry point on the concatenation of everything a slot was given, through joins and
clears of rows of many blocks; and one detect call with every reading flag on against the entry points on its own tables."""
import numpy as np
import pytest

import big_lexicon_cases as BC
import lattice_match_ref as LM
import lattice_track_ref as LT
import lexicon_layout as LL
import track_read_ref as TR
import word_match_ref as WM
from test_frame_lines import GROUPED
from test_lattice_decode_pipeline import proto  # noqa: F401  (the fixture)
from test_lattice_match_pipeline import BOTH, BAND, DEL, INS, lex  # noqa: F401  (the fixture)
from test_run_split_pipeline import SPLIT, _part_rows, scene  # noqa: F401  (the fixture)
from test_track_pool import EMPTY, as_pool

pytestmark = pytest.mark.gpu
SEVEN = ("entry", "cost", "second_entry", "second_cost", "free_cost", "n_tried", "n_used")


@pytest.fixture(scope="module")
def ctx(S):
    """A context per lexicon, made when a test first asks for it: every lexicon is built and set once."""
    made = {}

    def get(name):
        if name not in made:
            L = BC.lexicon(name)
            f = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
            f.set_lexicon(L.words, fold_case=L.fold)
            info = f.lexicon_info()
            assert info["n"] == L.lay.n and info["chunk_entries"] == LL.WM_GROUP * LL.WM_CHUNK_GROUPS and info["flags"] == int(L.fold)
            made[name] = f
        return made[name], BC.lexicon(name)

    yield get
    for f in made.values():
        f.close()


def _setup(S, f, c):
    ins, dele, band, split = c.setting
    f.set_word_match(ins, dele, band)
    f.set_run_split(1, 4, split)
    return ins, dele, band, split


def _rows(S, c, lattice):
    sp, rc, pc, first, n_of = c.rows(lattice)
    return sp.astype(S.RUN_SPLIT_DTYPE), rc, pc, first, n_of


def test_the_maximum_is_accepted_and_laid_out_as_the_mirror_says(ctx):
    f, L = ctx("max")
    assert f.lexicon_info()["n"] == LL.MAX_ENTRIES == len(L.words)
    # the image: goff, index, chars and pos behind the 512 bytes of the length tables, each rounded up to 256 bytes
    up = lambda x: -(-x // 256) * 256
    words32 = sum((int(L.lay.len_first[l + 1]) - int(L.lay.len_first[l])) * LL.WM_GROUP * ((l + 3) // 4) for l in range(1, 33))
    assert f.lexicon_info()["device_bytes"] >= up(up(up(512 + 4 * L.lay.n_groups) + 4 * L.lay.n_groups * LL.WM_GROUP) + 4 * words32) + 4 * L.lay.n


# ---- the track side ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["match_tracks", "lattice_match_tracks", "pool", "lattice_pool"])
@pytest.mark.parametrize("c", BC.TRACK_CASES, ids=repr)
def test_track_side(S, ctx, c, family):
    f, L = ctx(c.lex)
    ins, dele, band, split = _setup(S, f, c)
    lattice = family.startswith("lattice")
    sp, rc, pc, first, n_of = _rows(S, c, lattice)
    tf, tc, mem = BC.flat([c.track])
    want = BC.reference("track", c.name, lattice)
    assert want[0][0][:4] == c.wanted(lattice)
    if family == "match_tracks":
        rec, mc = f.match_tracks(rc, first, n_of, tf, tc, mem)
        hr, hm = S.match_tracks_host(rc, first, n_of, tf, tc, mem, L.words, L.fold, ins, dele, band)
        assert TR.as_tuples(rec) == want[0], (TR.as_tuples(rec), want[0])
        assert mc.tolist() == want[1].tolist()
        assert rec.tobytes() == hr.tobytes() and mc.tobytes() == hm.tobytes()
    elif family == "lattice_match_tracks":
        rec, mrec, src, parts = f.lattice_match_tracks(sp, rc, pc, first, n_of, tf, tc, mem)
        hr, hm, hs, hp = S.lattice_match_tracks_host(sp, rc, pc, first, n_of, tf, tc, mem, L.words, L.fold, ins, dele, band, split)
        assert LT.as_tuples(rec) == want[0], (LT.as_tuples(rec), want[0])
        assert LT.members_as_tuples(mrec) == want[1], (LT.members_as_tuples(mrec), want[1])
        assert (src == want[2]).all() and np.stack([parts["run"], parts["piece"]], 1).tolist() == want[3].tolist()
        assert rec.tobytes() == hr.tobytes() and mrec.tobytes() == hm.tobytes() and src.tobytes() == hs.tobytes() and parts.tobytes() == hp.tobytes()
        cut = [any(len(run) > 1 for run in c.words[w]) for w in mem]
        assert all((mrec["n_parts"][i] > n_of[w]) == cut[i] for i, w in enumerate(mem) if mrec["cost"][i] >= 0)          # the winner is read atom by atom
    else:
        pool = S.TrackPool(f, 3, lattice=lattice)
        try:
            half = len(mem) // 2                                   # the members in two calls, into the last slot
            for part in (mem[:half], mem[half:]):
                if lattice:
                    pool.add_lattice(sp, rc, pc, first, n_of, [0], [len(part)], part, [2])
                else:
                    pool.add(rc, first, n_of, [0], [len(part)], part, [2])
            got = pool.read([2, 0])
            if lattice:
                hr = S.lattice_match_tracks_host(sp, rc, pc, first, n_of, tf, tc, mem, L.words, L.fold, ins, dele, band, split)[0]
            else:
                hr = S.match_tracks_host(rc, first, n_of, tf, tc, mem, L.words, L.fold, ins, dele, band)[0]
            assert got[:1].tolist() == as_pool(S, hr, tc).tolist(), (got[0], hr[0])
            assert tuple(int(got[0][k]) for k in SEVEN) == want[0][0][:7] and tuple(got[1]) == EMPTY
            assert pool.info()["device_bytes"] >= 3 * 4 * LL.WM_GROUP * L.lay.n_groups
        finally:
            pool.close()


# ---- the word side ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["match_words", "lattice_match_words"])
@pytest.mark.parametrize("c", BC.WORD_CASES, ids=repr)
def test_word_side(S, ctx, c, family):
    f, L = ctx(c.lex)
    ins, dele, band, split = _setup(S, f, c)
    lattice = family.startswith("lattice")
    sp, rc, pc, first, n_of = _rows(S, c, lattice)
    want = BC.reference("word", c.name, lattice)
    if lattice:
        rec, src, parts = f.lattice_match_words(sp, rc, pc, first, n_of)
        hr, hs, hp = S.lattice_match_words_host(sp, rc, pc, first, n_of, L.words, L.fold, ins, dele, band, split)
        assert [r[:4] for r in want[0]] == c.wanted(True)
        assert LM.as_tuples(rec) == want[0], (LM.as_tuples(rec), want[0])
        assert (src == want[1]).all() and np.stack([parts["run"], parts["piece"]], 1).tolist() == want[2].tolist()
        assert rec.tobytes() == hr.tobytes() and src.tobytes() == hs.tobytes() and parts.tobytes() == hp.tobytes()
    else:
        rec = f.match_words(rc, first, n_of)
        assert [r[:4] for r in want] == c.wanted(False)
        assert WM.as_tuples(rec) == want, (WM.as_tuples(rec), want)
        assert rec.tobytes() == S.match_words_host(rc, first, n_of, L.words, L.fold, ins, dele, band).tobytes()


# ---- the pool on a long row -------------------------------------------------------------------------------------------------------
def _host(S, L, rows, lists, setting, lattice):
    ins, dele, band, split = setting
    tf, tc, mem = BC.flat(lists)
    if lattice:
        rec = S.lattice_match_tracks_host(*rows, tf, tc, mem, L.words, L.fold, ins, dele, band, split)[0]
    else:
        rec = S.match_tracks_host(*rows[1:2], *rows[3:], tf, tc, mem, L.words, L.fold, ins, dele, band)[0]
    return as_pool(S, rec, tc)


@pytest.mark.parametrize("lattice", [False, True], ids=["rows", "lattice"])
@pytest.mark.parametrize("name", ["pass2", "pass3"])
def test_pool_joins_and_clears_on_a_row_of_many_blocks(S, ctx, name, lattice):
    """The words of the lexicon's scenarios as one table (INS = 40, DEL = 90, under which the longer planted entry of every scenario
    wins; band 31: every length is read, so every block of a row counts): four slots in two additions each, a join of three sources, two clears, other members into the cleared slots and into a
    source of the join.  A block that k_pool_clear or k_pool_join left as it was keeps its sums: the planted winners of the members
    added afterwards lie in late blocks and would come out dearer than the host entry point has them."""
    f, L = ctx(name)
    setting = (40, 90, 31, BC.SPLIT)
    f.set_word_match(*setting[:3])
    f.set_run_split(1, 4, setting[3])
    cases = [c for c in BC.TRACK_CASES if c.lex == name and not c.free0]
    words = [w if lattice else BC.flatten(w) for c in cases for w in c.words]
    sp, rc, pc, first, n_of = BC.make_rows(words)
    rows = (sp.astype(S.RUN_SPLIT_DTYPE), rc, pc, first, n_of)
    nw = len(words)
    assert nw >= 5
    cap = 6
    pool = S.TrackPool(f, cap, lattice=lattice)

    def add(lists, slots):
        tf, tc, mem = BC.flat(lists)
        if lattice:
            pool.add_lattice(*rows, tf, tc, mem, slots)
        else:
            pool.add(rc, first, n_of, tf, tc, mem, slots)

    def check(lists):
        got, want = pool.read(list(range(cap))), _host(S, L, rows, lists, setting, lattice)
        assert got.tolist() == want.tolist(), [(s, tuple(a), tuple(b)) for s, (a, b) in enumerate(zip(got, want)) if tuple(a) != tuple(b)]
        return got

    try:
        assert pool.info()["device_bytes"] >= cap * 4 * LL.WM_GROUP * L.lay.n_groups
        lists = [[] for _ in range(cap)]
        first_call = [[0], [1, 2], [3 % nw], [4 % nw, 0]]
        second_call = [[1], [0], [2, 4 % nw], [3 % nw]]
        add(first_call, [0, 1, 2, 3])
        add(second_call, [3, 2, 1, 0])
        for s in range(4):
            lists[s] = first_call[s] + second_call[3 - s]
        got = check(lists)
        assert (got["entry"][:4] >= 0).all() and tuple(got[4]) == tuple(got[5]) == EMPTY
        pool.join(4, [0, 2, 3])                                # three sources into an empty slot
        lists[4], lists[0], lists[2], lists[3] = lists[0] + lists[2] + lists[3], [], [], []
        got = check(lists)
        assert tuple(got[0]) == tuple(got[2]) == tuple(got[3]) == EMPTY and got[4]["n_members"] == len(lists[4]) >= 6
        pool.clear([1, 4])
        lists[1], lists[4] = [], []
        last = nw - 1                                          # other members into the cleared slots and into a source of the join: no sum is left over
        add([[last], [last, 1], [0]], [1, 4, 2])
        lists[1], lists[4], lists[2] = [last], [last, 1], [0]
        got = check(lists)
        planted = {L.index[k] for k in L.index}
        assert all(int(got[s]["entry"]) in planted for s in (1, 2, 4))
        assert all(L.lay.tm_chunk_of[int(got[s]["entry"])] > 0 for s in (1, 4)), "the winners after the clear must lie behind the first block of the row"
    finally:
        pool.close()


# ---- the detect calls -------------------------------------------------------------------------------------------------------------
def test_a_list_call_with_every_reading_flag_on_a_lexicon_of_65_track_chunks(lex):  # noqa: F811
    """The scene and the prototype model of test_lattice_track_pipeline.py, every frame twice; the lexicon is the scene's own readings
    and background entries up to 65 chunks of 16 groups.  The call sizes its partial tables from the lexicon on a path of its own
    (api_run_read.cpp): its tables must be those of the entry points on the result's own rows, words and tracks."""
    S, g, prm, model, uniform, crops, words = lex
    T, G, V = LL.TM_CHUNK_GROUPS, LL.WM_GROUP, LL.WAVE
    need = V * T + 1 - LL.place(words).n_groups
    extra = {l: 0 for l in (2, 3, 4, 5, 6, 7, 8)}
    for i in range(need):                                      # whole groups of background, spread over the lengths 2 .. 8
        extra[2 + i % 7] += G
    more, _ = LL.build(extra, [], seed=11)
    big = list(words) + more
    lay = LL.place(big)
    assert lay.tm_chunks >= V + 1 and lay.n_groups >= V * T + 1
    frames = [uniform[0], uniform[0], uniform[1], uniform[1]]
    g.set_lexicon(big, fold_case=True)
    try:
        res = g.text_detect_list(frames, GROUPED, want_line_links=True, want_track_read=True, want_lattice_match=True, want_lattice_track=True, **BOTH)
        first, n_of = res.words["first_run"], res.words["n_runs"]
        tf, tc, mem = res.word_tracks["first"], res.word_tracks["count"], res.word_track_members
        assert len(first) > 0 and len(tf) > 0 and int(tc.max()) >= 2
        ws = res.word_splits
        part_rows = _part_rows(res)                            # word match and track read take the rows of the split parts
        wm = g.match_words(part_rows, ws["first_part"], ws["n_parts"])
        assert wm.tobytes() == res.word_matches.tobytes()
        tm, mc = g.match_tracks(part_rows, ws["first_part"], ws["n_parts"], tf, tc, mem)
        assert tm.tobytes() == res.track_matches.tobytes() and mc.tobytes() == res.track_member_costs.tobytes()
        lm = g.lattice_match_words(res.run_splits, res.run_costs, res.piece_costs, first, n_of)
        for a, b in zip((res.lattice_matches, res.lattice_match_src, res.lattice_match_parts), lm):
            assert a.tobytes() == b.tobytes()
        lt = g.lattice_match_tracks(res.run_splits, res.run_costs, res.piece_costs, first, n_of, tf, tc, mem)
        for a, b in zip((res.lattice_track_matches, res.lattice_track_members, res.lattice_track_src, res.lattice_track_parts), lt):
            assert a.tobytes() == b.tobytes()
        host = S.lattice_match_tracks_host(res.run_splits, res.run_costs, res.piece_costs, first, n_of, tf, tc, mem, big, True, INS, DEL, BAND, SPLIT)
        for a, b in zip(lt, host):
            assert a.tobytes() == b.tobytes()
        assert S.match_words_host(part_rows, ws["first_part"], ws["n_parts"], big, True, INS, DEL, BAND).tobytes() == wm.tobytes()
        for table in (res.word_matches, res.track_matches, res.lattice_matches, res.lattice_track_matches):
            e = table["entry"]
            assert ((e >= 0) & (e < len(words))).any() and (table["n_tried"] > len(words)).any()          # a reading of the scene wins, among background entries
    finally:
        g.set_lexicon(words, fold_case=True)
