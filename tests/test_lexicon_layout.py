"""The layout mirror (lexicon_layout.py) and the scenarios of test_big_lexicon.py without a GPU: place() against the library's own
placement loop restated entry by entry, the builder, the sizes of the five lexicons, and for every planted scenario that the planted
entries sit in the chunks, passes and lanes the scenario names and that the numpy references (word_match_ref, track_read_ref,
lattice_match_ref, lattice_track_ref) return the planted best and second at the costs worked out by hand -- equal costs included.  A
scenario that fails here is a mistake in the scenario, not in a kernel."""
import numpy as np
import pytest

import big_lexicon_cases as BC
import lexicon_layout as LL
import word_match_ref as WM

T, W, G, V = BC.T, BC.W, BC.G, BC.V


def test_the_constants_are_the_headers():
    assert LL.header_constant("word_match_kernels.h", "WM_GROUP") == G and LL.header_constant("track_match_kernels.h", "TM_CHUNK_GROUPS") == T
    assert G == LL.WAVE and W % T == 0 and T % 4 == 0                    # a lane an entry; a word-side chunk is whole track-side chunks


def test_place_equals_the_placement_loop_of_set_lexicon():
    rng = np.random.default_rng(1)
    words = ["".join(rng.choice(list(WM.ALPHABET), int(l))) for l in rng.choice([1, 2, 3, 5, 9, 32], 3000, p=[0.02, 0.3, 0.3, 0.3, 0.06, 0.02])]
    count = [0] * 34
    for w in words:
        count[len(w)] += 1
    len_first, len_count = [0] * 34, [0] * 34
    for l in range(1, 33):
        len_first[l + 1] = len_first[l] + (count[l] + G - 1) // G
        len_count[l + 1] = len_count[l] + count[l]
    index, placed = np.full((len_first[33], G), -1, np.int64), [0] * 34
    p = LL.place(words)
    for e, w in enumerate(words):
        slot = placed[len(w)]
        placed[len(w)] += 1
        g, lane = len_first[len(w)] + slot // G, slot % G
        index[g, lane] = e
        assert (p.slot[e], p.group[e], p.lane[e], p.tm_chunk_of[e], p.wm_chunk_of(e, 2)) == (slot, g, lane, g // T, (g - len_first[2]) // W)
    assert p.len_first.tolist() == len_first and p.len_count.tolist() == len_count and (p.index_image() == index).all()
    assert p.n_groups == len_first[33] and p.tm_chunks == -(-p.n_groups // T) and p.wm_chunks == -(-p.n_groups // W)
    assert [p.len_of_group(g) for g in range(p.n_groups)] == [l for l in range(1, 33) for _ in range(len_first[l + 1] - len_first[l])]
    assert LL.place([]).tm_chunks == LL.place([]).wm_chunks == 1


def test_the_builder_puts_the_planted_where_they_are_asked_and_draws_no_label_0():
    counts = {2: 70, 5: 130, 3: 64}
    planted = [("AB", 2, 69), ("CDEFG", 5, 0), ("HIJKL", 5, 64), ("000", 3, 63)]
    words, index_of = LL.build(counts, planted, (5, 2), seed=3)
    p = LL.place(words)
    assert len(words) == 264 and [len(w) for w in words] == [5] * 130 + [2] * 70 + [3] * 64          # the index order: 5, 2, then the rest ascending
    for text, l, slot in planted:
        e = index_of[l, slot]
        assert words[e] == text and p.slot[e] == slot and (p.group[e], p.lane[e]) == p.group_lane(l, slot) and p.slot_at(l, int(p.group[e]), int(p.lane[e])) == slot
    assert index_of[5, 0] == 0 and index_of[2, 69] == 130 + 69 and p.group[index_of[2, 69]] == 1 and p.group[index_of[5, 64]] == 2 + 1 + 1
    rest = [w for e, w in enumerate(words) if e not in index_of.values()]
    assert all(set(w) <= set(LL.BACKGROUND) for w in rest) and "0" not in LL.BACKGROUND and len(set(rest)) > 100
    assert LL.build(counts, planted, (5, 2), seed=3)[0] == words


@pytest.mark.parametrize("name,n_groups", [("full", V * T), ("pass2", V * T + 1), ("pass3", 2 * V * T + 1), ("word2", V * W + 1), ("max", LL.MAX_ENTRIES // G)])
def test_the_sizes_of_the_lexicons(name, n_groups):
    L = BC.lexicon(name)
    lay = L.lay
    assert lay.n_groups == n_groups and lay.tm_chunks == -(-n_groups // T) and lay.wm_chunks == -(-n_groups // W) and lay.n <= LL.MAX_ENTRIES
    assert (lay.count == L.plan.count).all() and all(L.words[e] == L.text[k] for k, e in L.index.items())
    assert not any("0" in w for w in L.words[::997]) and {len(w) for w in L.words} <= set(range(2, 9))
    if name == "full":
        assert lay.tm_chunks == V and n_groups % T == 0                       # the last full single pass
    if name == "pass2":
        assert lay.tm_chunks == V + 1 and n_groups % T == 1                   # the last chunk holds one group
    if name == "pass3":
        assert lay.tm_chunks == 2 * V + 1
    if name == "word2":
        assert lay.wm_chunks == V + 1 and n_groups % W == 1
    if name == "max":
        assert lay.n == LL.MAX_ENTRIES and (lay.count % G == 0).all() and lay.tm_chunks > 2 * V and lay.wm_chunks > 2 * V


def _where(L, key):
    e = L.index[key]
    return int(L.lay.group[e]), int(L.lay.lane[e]), int(L.lay.tm_chunk_of[e])


def _last_real_lane(L, key):
    """The entry sits in the last group, which is partial, in the last lane before the padding."""
    g, lane, _ = _where(L, key)
    img = L.lay.index_image()
    return g == L.lay.n_groups - 1 and lane < G - 1 and img[g, lane] == L.index[key] and (img[g, lane + 1:] == -1).all() and (img[g, :lane + 1] >= 0).all()


def _all_keys(c):
    """Every (cost, index) of the flattened words of a case at band 31, ascending: the third best."""
    L = BC.lexicon(c.lex)
    ins, dele, band, _ = c.setting
    assert band == 31
    sp, rc, pc, first, n_of = c.rows(False)
    members = c.track if c.side == "track" else [0]
    keys = []
    for l, (ix, E) in L.ref.by_len.items():
        tot = sum(WM.entry_costs((WM.fold_rows(rc[first[m]:first[m] + n_of[m]]) if L.fold else rc[first[m]:first[m] + n_of[m]]).astype(np.int64), E, ins, dele)
                  for m in members if n_of[m] <= 32)
        keys.append(np.stack([tot, ix], 1))
    keys = np.concatenate(keys)
    return keys[np.lexsort((keys[:, 1], keys[:, 0]))]


@pytest.mark.parametrize("c", BC.TRACK_CASES, ids=repr)
def test_track_side_scenarios_on_the_mirror_and_the_references(c):
    L = BC.lexicon(c.lex)
    lay, idx = L.lay, L.index
    chunk = lambda key: _where(L, key)[2]
    if c.name == "full":
        assert chunk("HI") == V - 1 == lay.tm_chunks - 1 and chunk("LO") == 0
    if c.name in ("P1", "P2"):
        lo, hi = chunk("P12.LO"), chunk("P12.HI")
        assert hi == lo + V and LL.merge_lane_pass(lo) == (lo, 0) and LL.merge_lane_pass(hi) == (lo, 1)          # one lane, consecutive passes
        assert c.want[0] == ("P12.LO" if c.name == "P1" else "P12.HI")
    if c.name == "P4_P8":
        assert chunk("P4.BEST") == lay.tm_chunks - 1 and lay.n_groups % T != 0 and _last_real_lane(L, "P4.BEST") and c.free0
        assert chunk("P4.SECOND") < lay.tm_chunks - 1
    if c.name == "P3":
        assert chunk("P3.BEST") == chunk("P3.SECOND") >= V and chunk("P3.THIRD") == chunk("P3.BEST") - V
        assert _where(L, "P3.BEST")[0] != _where(L, "P3.SECOND")[0]           # (two groups of the chunk: two waves of k_track_match)
        third = _all_keys(c)[2]
        assert third.tolist() == [216, idx["P3.THIRD"]]                       # 3 members of 4 h + DEL
    if c.name == "P5":
        assert idx["P5.LONG"] < idx["P5.SHORT"] and chunk("P5.LONG") - chunk("P5.SHORT") >= V
        assert LL.merge_lane_pass(chunk("P5.LONG"))[0] == LL.merge_lane_pass(chunk("P5.SHORT"))[0]
        assert c.setting[0] == c.setting[1]                                   # INS = DEL
    if c.name in ("P6", "P6max"):
        spots = [LL.merge_lane_pass(chunk(k)) for k in ("P6.A", "P6.B", "P6.C")]
        assert len({s[0] for s in spots}) == 1 and len({s[1] for s in spots}) == 3 and spots[0][1] < spots[1][1] < spots[2][1]
        assert idx["P6.C"] < idx["P6.A"] < idx["P6.B"] and c.setting[0] == c.setting[1]
        if c.name == "P6":
            assert [chunk(k) for k in ("P6.A", "P6.B", "P6.C")] == [0, V, 2 * V]
        else:
            first_tried = lay.tm_chunk(int(lay.len_first[5]))
            assert c.setting[2] == 1 and first_tried >= V                   # every chunk of the first passes holds no key
    # the run counts across the cases: the three buckets, an unusable member, cut and uncut members in lattice mode
    for lattice in (False, True):
        rec, *rest = BC.reference("track", c.name, lattice)
        assert len(rec) == 1 and rec[0][:4] == c.wanted(lattice), (lattice, rec[0], c.wanted(lattice))
        assert rec[0][6] == sum(1 for w in c.words if len(w) <= 32)
    if c.name in ("P5", "P6", "P6max"):
        assert c.wanted(False)[1] == c.wanted(False)[3] and c.wanted(True)[1] == c.wanted(True)[3] and c.wanted(True)[0] < c.wanted(True)[2]


def test_the_track_cases_cover_the_run_counts():
    runs = sorted({len(BC.flatten(w)) for c in BC.TRACK_CASES for w in c.words})
    assert any(r <= 8 for r in runs) and any(8 < r <= 16 for r in runs) and any(16 < r <= 32 for r in runs) and any(r > 32 for r in runs)
    for c in BC.TRACK_CASES:
        cut = [any(len(run) > 1 for run in w) for w in c.words if len(w) <= 32]
        assert any(cut) and not all(cut), c                                   # lattice mode: cut and uncut members in every track
    assert any(len(run) == 4 for c in BC.TRACK_CASES for w in c.words for run in w)          # ... and a run of three cuts


@pytest.mark.parametrize("c", BC.WORD_CASES, ids=repr)
def test_word_side_scenarios_on_the_mirror_and_the_references(c):
    L = BC.lexicon(c.lex)
    lay, idx = L.lay, L.index
    band = c.setting[2]
    # the band's first length: the run count less the band (the word uncut, and with a run of two atoms: one run fewer)
    for w in c.words:
        len_lo = max(1, len(w) - band)
        base = int(lay.len_first[len_lo])
        chunk = lambda key: lay.wm_chunk_of(idx[key], len_lo)
        assert base == int(lay.len_first[max(1, len(c.words[0]) - band)])     # both words count their chunks from the same group
        if c.name in ("P1", "P2"):
            assert base == 0 and chunk("P12.LO") == 0 and chunk("P12.HI") == V and c.want[0][0] == ("P12.LO" if c.name == "P1" else "P12.HI")
        if c.name == "P3":
            assert chunk("P3.BEST") == chunk("P3.SECOND") == V and chunk("P3.THIRD") == 0
        if c.name == "P4":
            assert chunk("P4.BEST") == lay.wm_chunks - 1 == V and lay.n_groups % W != 0 and _last_real_lane(L, "P4.BEST") and c.free0 and chunk("P4.SECOND") < V
        if c.name == "P5":
            assert idx["P5.LONG"] < idx["P5.SHORT"] and chunk("P5.LONG") == V and chunk("P5.SHORT") == 0 and c.setting[0] == c.setting[1]
        if c.name == "P6max":
            r = [chunk(k) for k in ("P6.A", "P6.B", "P6.C")]
            assert r[1] == r[0] + V and r[2] == r[0] + 2 * V and base % W != 0 and idx["P6.C"] < idx["P6.A"] < idx["P6.B"]
        if c.name == "ENDSmax":
            g, lane, _ = _where(L, "ENDS.BEST")
            assert (g, lane) == (lay.n_groups - 1, G - 1) and lay.n == LL.MAX_ENTRIES and _where(L, "ENDS.SECOND")[:2] == (base, 0) and base > V * W
        if c.name == "P7max":
            gb, gs = _where(L, "P7.BEST")[0], _where(L, "P7.SECOND")[0]
            assert base % W != 0 and (gb - base) % W == 0 and gs == gb - 1 and chunk("P7.SECOND") == chunk("P7.BEST") - 1 >= 0
            assert gb // W == gs // W                                         # counted from group 0 they would share a chunk
    if c.name == "P3":
        assert _all_keys(c)[2].tolist() == [136, idx["P3.THIRD"]]            # 4 h + 2 DEL
    for lattice in (False, True):
        rec = BC.reference("word", c.name, lattice)
        rec = rec[0] if lattice else rec
        assert [r[:4] for r in rec] == c.wanted(lattice), (lattice, rec, c.wanted(lattice))
    if c.name in ("P5", "P6max"):
        assert all(w[1] == w[3] and w[0] < w[2] for w in c.wanted(True))
