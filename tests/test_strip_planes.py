"""The CPU half of the strip path's edge tests: every plane of tests/strip_planes.py is what it was built for, by the cut census (numpy and scipy, no
kernel); `cut_rows` against its brute-force form; the sentinel rule of str_er_strip_extract_dev stated in float32.  tests/test_strip_edges.py runs the
same planes through the library."""
import numpy as np
import pytest

import strip_planes as sp
import tree_planes as tp

CASES = sp.cases()


def _census(name, step=8):
    plane, n = CASES[name]
    return sp.CutCensus(plane, step, n)


def _of(kind):
    return [k for k in CASES if k.split("/")[0] == kind]


# ---- the cut -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", list(range(1, 131)) + [2160])
def test_cut_rows_against_the_brute_force_form(h):
    """Every tile row belongs to exactly one strip -- the one whose interval [i * ty // n, (i + 1) * ty // n) holds it --, the intervals are monotone, and
    with more strips than tile rows exactly n - ty strips are empty."""
    ty = -(-h // 32)
    for n in sorted({1, 2, 3, ty, ty + 1, 2 * ty + 1, 5, 8}):
        strips = sp.cut_rows(h, n)
        assert len(strips) == n
        owner = [[i for i in range(n) if (i * ty) // n <= t < ((i + 1) * ty) // n] for t in range(ty)]
        assert all(len(o) == 1 for o in owner)                              # covered once
        flat = [o[0] for o in owner]
        assert flat == sorted(flat)                                          # monotone
        for i, s in enumerate(strips):
            mine = [t for t in range(ty) if flat[t] == i]
            assert (s.t1 - s.t0) == len(mine) and (not mine or (s.t0, s.t1) == (mine[0], mine[-1] + 1))
            assert s.rows == sum(min(32, h - 32 * t) for t in mine)
            assert s.has_top == (bool(mine) and mine[0] > 0) and s.has_bot == (bool(mine) and mine[-1] < ty - 1)
            assert s.row0 == (32 * (s.t0 - 1) if s.t0 > 0 else 0)
        assert sum(s.rows for s in strips) == h
        assert sum(1 for s in strips if s.rows == 0) == max(0, n - ty)
        if n == 2 * ty + 1 and ty > 1:
            # strips without rows lie BETWEEN strips with rows: the merge's walk from `lo` to the next strip with a top row skips them
            live = [i for i, s in enumerate(strips) if s.rows]
            assert any(b - a > 1 for a, b in zip(live, live[1:]))
        assert [r for r, _, _ in sp.cuts(h, n)] == sorted({s.r0 for s in strips if s.rows and s.r0 > 0})


def test_strip_counts_and_heights_reach_what_they_are_for():
    s = sp.cut_rows(33, 2)
    assert (s[1].r0, s[1].rows, s[1].row0, s[1].has_top, s[1].has_bot) == (32, 1, 0, True, False)        # a last strip of one row behind a phantom row
    for h in sp.HEIGHTS:
        ty = sp.tile_rows(h)
        assert sp.strip_counts(h) == sorted({1, 2, ty, ty + 1, 2 * ty + 1})
        assert sp.cuts(h, 1) == []
        inner = [x for x in sp.cut_rows(h, ty) if x.has_top and x.has_bot]
        assert len(inner) == max(0, ty - 2) and all(x.rows == 32 for x in inner)          # a strip a tile row: every inner strip has both phantom rows
        assert sum(1 for x in sp.cut_rows(h, ty + 1) if x.rows == 0) == 1
    seen = {}
    for name, (p, n) in CASES.items():
        h, w = p.shape
        ty = sp.tile_rows(h)
        for what, val in (("1", 1), ("2", 2), ("ty", ty), ("ty+1", ty + 1), ("2ty+1", 2 * ty + 1)):
            if n == val:
                seen.setdefault(what, set()).add(name.split("/")[0])
        assert w in sp.WIDTHS and h in sp.HEIGHTS, name
    assert all(len(v) >= 2 for v in seen.values()) and set(seen) == {"1", "2", "ty", "ty+1", "2ty+1"}, seen
    for kind in {k.split("/")[0] for k in CASES} - {"flat0"}:
        ws = {CASES[k][0].shape[1] for k in _of(kind)}
        assert min(ws) < 64 < max(ws) and any(w < 256 for w in ws) and any(w > 256 for w in ws) or kind == "levels_on64", (kind, ws)
    ws = {CASES[k][0].shape[1] for k in _of("levels_on64")}
    assert any(w < 256 for w in ws) and any(w > 256 for w in ws)


# ---- the sentinel rule ----------------------------------------------------------------------------------------------------------
def test_sentinel_rule_in_float32():
    """str_er_strip_extract_dev takes a thresh step iff lrintf(255.0f * (float)(1.0 / step)) == 255 / step + 1: the pixel value 255 must land on the wall
    level, which the flood never enters.  FINDING: the accepted steps up to 32 are NOT the powers of two alone.  The rule holds wherever the fraction of
    255 / step is above a half, or is exactly a half and rounds to even upwards: 10 (25.5 -> 26), 13, 20, 22, 24, 26 and 29 are accepted as well; 6 (42.5
    -> 42) and 30 (8.5 -> 8) are exact halves that round down, and 1, 3, 5, 15, 17 divide 255.  The GPU half runs the strip path at every step of ACCEPTED."""
    accepted = [s for s in range(1, 33) if sp.step_accepted(s)]
    assert {2, 4, 8, 16, 32} <= set(accepted)
    assert accepted == [2, 4, 8, 10, 13, 16, 20, 22, 24, 26, 29, 32]
    assert not any(sp.step_accepted(s) for s in (1, 3, 6))
    for s in accepted:
        q, hi = tp.quantise(np.array([[255, 0, 64, 128]], np.uint8), s)
        assert int(q[0, 0]) == hi and len({int(x) for x in q[0, 1:]}) == 3 and int(q[0, 3]) < hi        # 255 is a wall; 0 / 64 / 128 are three levels below it
    # the rule in exact arithmetic agrees with the float32 form on every step up to 32 but the exact halves, where half-to-even decides
    for s in range(1, 33):
        frac = (255 % s) / s
        if frac != 0.5:
            assert sp.step_accepted(s) == (frac > 0.5), s


ACCEPTED = [s for s in range(1, 33) if sp.step_accepted(s)]


# ---- every plane reaches the case it is named for --------------------------------------------------------------------------------
def test_gray_frames_carry_the_plane():
    p = CASES["serpent/63x33/2"][0]
    f = sp.frame_of(p)
    assert f.shape == (33, 63, 3) and all((f[:, :, c] == p).all() for c in range(3))
    assert 1868 + 9617 + 4899 == 16384


def test_bar_and_flat_runs():
    for name in _of("bar") + _of("flat"):
        c = _census(name)
        p, n = CASES[name]
        w = p.shape[1]
        assert len(c.cuts) == len(sp.cuts(p.shape[0], n))
        for cut in c.cuts:
            assert cut.pairs == w
            assert cut.straddles == {x for x in (64, 256) if x < w}, name          # one run of equal pairs across 63 | 64 and 255 | 256
            if name.startswith("flat"):
                assert cut.node_pairs == 1 and cut.longest_run == w
            else:
                assert cut.node_pairs == 2 and cut.longest_run >= (w - 3) // 2
                assert cut.crossings == {0: [1], 16: [1]} and cut.multi() == 0      # the bar and the ground cross every cut once
        if name.startswith("bar"):
            assert c.key_rows() == {0: [0], 16: [0]}                                # both keys lie in strip 0
    assert any(len(_census(k).cuts) == 0 for k in _of("bar")) and any(len(_census(k).cuts) == 3 for k in _of("bar"))


def test_stripes_have_no_equal_neighbours():
    for name in _of("stripes"):
        c = _census(name)
        w = CASES[name][0].shape[1]
        assert c.cuts
        for cut in c.cuts:
            assert cut.longest_run == 1 and cut.pairs == w and cut.straddles == set()
            assert cut.node_pairs == (w + 1) // 2 + 1                               # every dark stripe a pair of its own, and the ground's
            assert cut.crossings[0] == [1] * ((w + 1) // 2)                         # w / 2 regions, each crossing once


def test_serpent_is_one_region_crossing_many_times():
    for step in (8, 2, 32):
        for name in _of("serpent"):
            c = _census(name, step)
            p, n = CASES[name]
            h, w = p.shape
            assert c.cuts
            lab, n_dark = tp.ndimage.label(p == sp.DARK)
            for cut in c.cuts:
                many = [x for x in cut.crossings[0] if x >= w / 4]
                assert len(many) == 1 and many[0] >= (w - 3) // 2 and cut.multi() == 1, name        # ONE region, crossing at every even column
                assert cut.longest_run == 1
                # its pieces above meet only through the pieces below and the other way round: w / 4 nodes on either side, a chain of unions
                above = {int(x) for x in cut.above if x >= 0 and (x >> 32) == 0}
                below = {int(x) for x in cut.below if x >= 0 and (x >> 32) == 0}
                assert len(above) >= w // 4 and len(below) >= w // 4, name
            assert n_dark <= len(c.cuts) * 2                                          # (a clipped last piece at most, beside the serpent of each cut)
            assert c.key_rows()[0][0] == c.cuts[0].row - min(3, 32)                   # the key: the first pixel of the topmost piece ABOVE the first cut


def test_u_shapes():
    for name in _of("u") + _of("u_mirror"):
        c = _census(name)
        p, n = CASES[name]
        cut = c.cuts[0]
        assert cut.crossings[0] == [2] and cut.multi() == 1 and cut.max_crossings() == 2, name         # one region, crossing twice
        dark_above = {int(x) for x in cut.above if x >= 0 and (x >> 32) == 0}
        dark_below = {int(x) for x in cut.below if x >= 0 and (x >> 32) == 0}
        mirror = name.startswith("u_mirror")
        assert (len(dark_above), len(dark_below)) == ((1, 2) if mirror else (2, 1)), name
        assert c.key_rows()[0][0] < cut.row                                           # the key pixel is in the upper strip
        if mirror and p.shape[0] >= 64:
            assert (p[cut.row:] == sp.DARK).sum() > (p[:cut.row] == sp.DARK).sum()    # ... although most of the area is below
    for name in _of("u_three"):
        c = _census(name)
        a, b = c.cuts[0], c.cuts[1]
        assert a.crossings[0] == [2] and b.crossings[0] == [2] and b.hi - a.lo >= 2, name
        mid = c.strips[a.hi]
        lab, k = tp.ndimage.label(CASES[name][0][mid.r0:mid.r1] == sp.DARK)
        assert k == 2 and a.hi == b.lo                                                # two separate arms through the whole middle strip


def test_rings_are_nested_on_both_sides():
    for name in _of("rings8") + _of("rings8_wall20"):
        c = _census(name)
        p, n = CASES[name]
        h, w = p.shape
        cut = c.cuts[0]
        lv_above = {int(x) >> 32 for x in cut.above if x >= 0}
        lv_below = {int(x) >> 32 for x in cut.below if x >= 0}
        depth = min(31, w // 2 - (1 if w % 2 == 0 else 0)) + 1
        walls = name.startswith("rings8_wall20")
        assert lv_above == lv_below and len(lv_above) >= min(31, w // 2 - 1) - (1 if walls else 0), (name, depth)
        assert (p[cut.row - 1, w // 2], p[cut.row, w // 2]) == (0, 0)                 # the centre lies on the cut
        if walls:
            assert (c.wall[cut.row - 1] & c.wall[cut.row]).sum() == 2                 # the ring of walls crosses the cut twice
            lab, k = tp.ndimage.label(~c.wall)
            assert k == 2 and lab[0, 0] != lab[cut.row, w // 2]                       # and seals its inside off
        else:
            assert all(v == [1] for v in cut.crossings.values())                      # every level set crosses the cut in one run
    # the step-2 form: the deepest nesting the step allows
    for w, h, n in ((257, 97, 4), (65, 64, 2)):
        c = sp.CutCensus(sp.rings(w, h, n, 2, 127, cut=len(sp.cuts(h, n)) // 2), 2, n)
        assert c.hi == 128 and not c.wall.any()
        assert len(np.unique(c.q)) == min(127, w // 2) + 1
    assert len(np.unique(tp.quantise(sp.rings(257, 97, 4, 2, 127, cut=1), 2)[0])) == 128      # levels 0 .. 127 of step 2: all of them


def test_levels_across_in_the_chosen_order():
    for name in _of("levels") + _of("levels_on64"):
        c = _census(name)
        p, n = CASES[name]
        w = p.shape[1]
        for cut in c.cuts:
            a, b = c.q[cut.row - 1], c.q[cut.row]
            sign = np.sign(a.astype(int) - b.astype(int))
            change = [int(x) for x in np.flatnonzero(np.diff(sign)) + 1]
            assert [int(sign[0])] + [int(sign[x]) for x in change] == [-1, 0, 1][:len(change) + 1], name
            if name.startswith("levels_on64"):
                assert change == ([64, 256] if w > 256 else [64, 128]), name          # the thirds begin on a wave's first lane
            else:
                assert change == [w // 3, 2 * w // 3] and all(x % 64 for x in change), name
            assert cut.node_pairs == 3 and cut.pairs == w


def test_corners_stay_apart():
    seen = set()
    for name in _of("corner") + _of("corner_b"):
        c = _census(name)
        p, n = CASES[name]
        w = p.shape[1]
        assert c.cuts
        xs = sp.corner_columns(w, "b" if name.startswith("corner_b") else "a")
        assert {0, w - 2} & set(xs) and len(xs) >= 2
        seen |= set(xs) if w > 66 else set()
        for cut in c.cuts:
            assert 0 not in cut.crossings                                              # no dark region crosses
            assert [int(x) for x in np.flatnonzero(p[cut.row - 1] == 0)] == sorted(xs)
            assert [int(x) for x in np.flatnonzero(p[cut.row] == 0)] == sorted(x + 1 for x in xs)
            assert cut.node_pairs == 1 + 2 * len(xs)                                   # (ground, ground), (dark, ground) and (ground, dark) for every corner
        lab, k = tp.ndimage.label(p == 0)
        assert k == 2 * len(xs) * len(c.cuts)                                          # every dark pixel a region of its own
    assert {0, 62, 63, 64, 253, 255} <= seen                                           # between them the two planes hold every x the corners are meant for


def test_wall_cuts():
    for kind in ("above", "both", "below"):
        for name in _of("wall_" + kind):
            for step in (8, 2, 32):
                c = _census(name, step)
                p, n = CASES[name]
                w = p.shape[1]
                assert c.cuts
                for cut in c.cuts:
                    if kind == "below":
                        walls = set(np.flatnonzero(c.wall[cut.row]).tolist())
                        assert {x for x in (0, 63, 64, w - 1) if x < w} <= walls and set(range(1, w, 2)) <= walls
                        assert cut.pairs == w - len(walls) > 0 and not c.wall[cut.row - 1].any()
                        assert cut.longest_run == 1                                    # (no two neighbouring pairs at all)
                    else:
                        assert cut.pairs == 0 and cut.node_pairs == 0 and cut.crossings == {}
                        assert c.wall[cut.row - 1].all() and c.wall[cut.row].all() == (kind == "both")
                if kind != "below":
                    assert tp.ndimage.label(~c.wall)[1] == sum(1 for k in c.nonwall if k > 0) >= 1      # every strip with a pixel left is sealed off from the others


def test_empty_strips():
    for name in _of("empty"):
        c = _census(name)
        p, n = CASES[name]
        dead = [i for i, s in enumerate(c.strips) if s.rows and c.nonwall[i] == 0]
        assert len(dead) == 1 and c.strips[dead[0]].has_top and c.strips[dead[0]].has_bot, name
        assert all(cut.pairs == 0 for cut in c.cuts if dead[0] in (cut.lo, cut.hi))
        inv = sp.CutCensus(CASES[name.replace("empty", "empty_inverted")][0], 8, n)
        s = inv.strips[dead[0]]
        assert (inv.q[s.r0:s.r1] == 0).all() and not inv.wall[s.r0:s.r1].any()        # the complement: one flat region of level 0
        for cut in inv.cuts:
            if dead[0] in (cut.lo, cut.hi):
                assert cut.pairs > 0 and len({int(x) for x in (cut.below if cut.lo != dead[0] else cut.above) if x >= 0}) == 1


def test_step_cases_keep_their_levels_at_every_accepted_step():
    for step in ACCEPTED:
        cs = sp.step_cases(step)
        assert {k.split("/")[0].split("_")[0] for k in cs} == set(sp.STEP_UNIT_KINDS)
        for name, (p, n) in cs.items():
            c = sp.CutCensus(p, step, n)
            assert c.cuts, name
            if name.startswith("rings"):
                walled = name.startswith("rings_wall")
                # as many rings as the step has levels below the wall level (and as 65 columns hold), and the centre; a ring of walls takes one away
                assert len(np.unique(c.q[~c.wall])) == min(255 // step, p.shape[1] // 2) + 1 - walled, (step, name)
                assert c.wall.any() == walled
            elif name.startswith("serpent"):
                assert all(max(cut.crossings[0]) >= (p.shape[1] - 3) // 2 for cut in c.cuts)
            elif name.startswith("levels"):
                assert all(cut.node_pairs == 3 for cut in c.cuts)
            elif name.startswith("wall_below"):
                assert all(0 < cut.pairs < p.shape[1] // 2 + 1 for cut in c.cuts)
            else:
                assert all(cut.pairs == 0 for cut in c.cuts)


def test_big_strips_hold_more_records_than_one_grid_round():
    """32 x 36 tiles of 965 nodes each, every one exported whichever tile kernel runs: more than the 4096 x 256 records one launch of k_rebase_records or
    k_check_forest covers without its grid-stride loop -- and every tile holds a region that is kept at MIN_AREA 120."""
    t = sp.big_tile()
    c = tp.Census(tp.positions_plane(t), 8, 120)
    n = sp.BIG_TILE_NODES
    assert [int(c.nodes()[i, i]) for i in range(3)] == [n] * 3 and n > tp.DENSE_FOLD > tp.SPARSE_FOLD
    assert [int(c.exported(tp.SPARSE_FOLD)[i, i]) for i in range(3)] == [n] * 3 == [int(c.exported(tp.DENSE_FOLD)[i, i]) for i in range(3)]
    lab, k = tp.ndimage.label(t <= sp.MID)
    assert int(np.bincount(lab.ravel())[1:].max()) > 120 and (t[0] != sp.MID).all() and (t[:, 0] != sp.MID).all()       # the block with the speckles in it: closed, and kept
    p = sp.big_strips_plane()
    assert p.shape == (2304, 2048)
    s = sp.cut_rows(p.shape[0], 2)
    assert (s[0].rows, s[1].r0, s[1].rows) == (1152, 1152, 1152)
    assert (p.reshape(72, 32, 32, 64).transpose(0, 2, 1, 3) == t).all()
    assert sp.BIG_TILES_X * sp.BIG_TILE_ROWS * n == 1111680 > 4096 * 256 == 1 << 20


def test_case_count():
    """161 (plane, size, strips) cases at thresh step 8 and 114 over the twelve accepted steps, each run at MIN_AREA 120 and 1."""
    assert len(CASES) == 161
    assert [len(sp.step_cases(s)) for s in ACCEPTED] == [10] * 6 + [9] * 6       # (from step 20 up a step has too few levels for the ring of walls)
    assert sorted({n for _, n in CASES.values()}) == [1, 2, 3, 4, 5, 7, 9]
