"""Planes made up for the strip path (api_strips.cpp: str_er_strip_extract[_dev], str_er_strip_merge[_ex]; er_tree_passes.inl: k_strip_border_ids,
k_rebase_records, k_check_forest, k_connect_cut), and a CPU census that says what a plane puts on a cut.

`cut_rows` restates the cut from the header comment of api_strips.cpp: a plane of h rows has ty_all = ceil(h / 32) tile rows, strip i of n holds the tile
rows [i * ty_all // n, (i + 1) * ty_all // n).  `CutCensus` derives everything else from the definition of the component tree -- numpy and
scipy.ndimage.label, no kernel: the node of a pixel inside a strip is the component of {level <= its own level} of THAT STRIP's rows which holds it, a
pixel pair across a cut joins the node above with the node below, and a region of the whole plane crosses a cut once for every run of columns in which
it holds both pixels of the pair.  Levels and walls are tree_planes.quantise's.

The builders return uint8 planes; a frame is the plane as gray BGR (b = g = r = v), for which the colour conversion gives Y = v exactly
(1868 + 9617 + 4899 = 16384) and Cr = Cb = 128: channel_mask 0x09 is the plane and its complement 255 - v.  Every builder puts its structure on every cut
of the strip count it is given; tests/test_strip_planes.py asserts with the census that it does.
"""
import numpy as np
from scipy import ndimage

import tree_planes as tp

TILE_H = tp.TILE_H
GROUND, MID, DARK, WALL = 128, 64, 0, 255        # levels 4, 2, 0 at thresh step 32 and distinct at every smaller step; 255 is a wall at every accepted step
WIDTHS = (1, 63, 64, 65, 255, 256, 257)
HEIGHTS = (33, 64, 65, 96, 97)


def rint_half_even(x):
    return float(np.rint(x))


def step_accepted(step):
    """The sentinel rule of str_er_strip_extract_dev in float32, as the host computes it: the pixel value 255 lands on the wall level."""
    return int(rint_half_even(np.float32(255) * np.float32(1.0 / step))) == 255 // step + 1


def tile_rows(h):
    return -(-h // TILE_H)


def strip_counts(h):
    """The strip counts the issue names: no cut, one cut, a strip a tile row, one strip more than tile rows, empty strips between strips with rows."""
    t = tile_rows(h)
    return sorted({1, 2, t, t + 1, 2 * t + 1})


class Strip:
    __slots__ = ("t0", "t1", "r0", "r1", "rows", "row0", "has_top", "has_bot")

    def __repr__(self):
        return "Strip(rows [%d, %d), row0 %d, top %d, bot %d)" % (self.r0, self.r1, self.row0, self.has_top, self.has_bot)


def cut_rows(h, n_strips):
    """One Strip per strip: tile rows [t0, t1), pixel rows [r0, r1), `rows` of them; row0 = the plane row of the strip's own row 0 (the phantom tile row
    above it where the plane goes on above); has_top / has_bot: it has rows and the plane goes on above / below them."""
    ty_all = tile_rows(h)
    out = []
    for i in range(n_strips):
        s = Strip()
        s.t0, s.t1 = i * ty_all // n_strips, (i + 1) * ty_all // n_strips
        s.r0, s.r1 = s.t0 * TILE_H, min(h, s.t1 * TILE_H)
        s.rows = max(0, s.r1 - s.r0)
        s.row0 = s.r0 - TILE_H if s.r0 > 0 else 0
        s.has_top = s.rows > 0 and s.r0 > 0
        s.has_bot = s.rows > 0 and s.r1 < h
        out.append(s)
    return out


def cuts(h, n_strips):
    """[(row, strip above, strip below)]: the cuts between two strips that have rows; `row` is the first row below the cut."""
    live = [(i, s) for i, s in enumerate(cut_rows(h, n_strips)) if s.rows > 0]
    return [(b.r0, i, j) for (i, a), (j, b) in zip(live, live[1:])]


def frame_of(plane):
    return np.ascontiguousarray(np.repeat(np.asarray(plane, np.uint8)[:, :, None], 3, axis=2))


def row_nodes(q, wall, row):
    """Node of every pixel of one row of a strip (q, wall: the strip's rows only): level << 32 | label of its component of {L <= level}; -1: a wall."""
    out = np.full(q.shape[1], -1, np.int64)
    for t in np.unique(q[row][~wall[row]]):
        lab, _ = ndimage.label((q <= t) & ~wall)
        sel = (q[row] == t) & ~wall[row]
        out[sel] = (int(t) << 32) + lab[row][sel].astype(np.int64)
    return out


class Cut:
    """What one cut carries: `pairs` pixel pairs with both sides not walls, `node_pairs` distinct (node above, node below) among them, `longest_run`
    of equal neighbouring pairs (1: no two neighbours are equal; 0: no pair at all), `straddles` = the x of {64, 256} for which one run of equal pairs
    holds x - 1 and x, `crossings` = level -> how often every region of the whole plane with that level crosses the cut (regions that do not are
    left out)."""
    __slots__ = ("row", "lo", "hi", "pairs", "node_pairs", "longest_run", "straddles", "crossings", "above", "below")

    def multi(self):
        return sum(1 for v in self.crossings.values() for c in v if c > 1)

    def max_crossings(self):
        return max((c for v in self.crossings.values() for c in v), default=0)


class CutCensus:
    def __init__(self, plane, step, n_strips):
        plane = np.asarray(plane, np.uint8)
        self.h, self.w = plane.shape
        self.step, self.n_strips = step, n_strips
        self.q, self.hi = tp.quantise(plane, step)
        self.wall = self.q >= self.hi
        self.strips = cut_rows(self.h, n_strips)
        self.nonwall = [int((~self.wall[s.r0:s.r1]).sum()) if s.rows else 0 for s in self.strips]
        self.cuts = []
        whole = self._whole_plane_labels() if cuts(self.h, n_strips) else []
        for r, lo, hi in cuts(self.h, n_strips):
            a, b = self.strips[lo], self.strips[hi]
            c = Cut()
            c.row, c.lo, c.hi = r, lo, hi
            c.above = row_nodes(self.q[a.r0:a.r1], self.wall[a.r0:a.r1], a.rows - 1)
            c.below = row_nodes(self.q[b.r0:b.r1], self.wall[b.r0:b.r1], 0)
            ok = (c.above >= 0) & (c.below >= 0)
            c.pairs = int(ok.sum())
            c.node_pairs = len({(int(x), int(y)) for x, y in zip(c.above[ok], c.below[ok])})
            same = ok[1:] & ok[:-1] & (c.above[1:] == c.above[:-1]) & (c.below[1:] == c.below[:-1])        # same[x - 1]: pair x equals pair x - 1
            run = best = 1 if c.pairs else 0
            for x in range(1, self.w):
                run = run + 1 if same[x - 1] else 1
                if ok[x]:
                    best = max(best, run)
            c.longest_run = best
            c.straddles = {x for x in (64, 256) if x < self.w and same[x - 1]}
            c.crossings = {}
            for t, lab, nodes in whole:
                both = (lab[r - 1] > 0) & (lab[r] > 0)
                starts = both & ~np.concatenate(([False], both[:-1]))
                counts = np.bincount(lab[r][starts], minlength=int(lab.max()) + 1)
                got = [int(counts[i]) for i in nodes if counts[i] > 0]
                if got:
                    c.crossings[t] = got
            self.cuts.append(c)

    def _whole_plane_labels(self):
        out = []
        for t in np.unique(self.q[~self.wall]):
            lab, _ = ndimage.label((self.q <= t) & ~self.wall)
            nodes = np.unique(lab[(self.q == t) & ~self.wall])         # the components that hold a level-t pixel: the regions of level t
            out.append((int(t), lab, nodes))
        return out

    def key_rows(self):
        """level -> rows of the key pixels (first own-level pixel in raster order) of the whole plane's regions of that level."""
        out = {}
        for t, lab, nodes in self._whole_plane_labels():
            own = np.flatnonzero(((self.q == t) & ~self.wall).ravel())
            _, first = np.unique(lab.ravel()[own], return_index=True)
            out[t] = sorted(int(own[i]) // self.w for i in first)
        return out


# =================================================================================================================================
# builders: (w, h, n_strips) -> plane.  Each puts its structure on EVERY cut of cuts(h, n_strips).
# =================================================================================================================================
def _band(r, h, depth):
    """Rows [r - a, r + b) around the cut at r, at most `depth` on either side, inside the strips next to the cut's tile rows."""
    return max(r - depth, r - TILE_H, 0), min(r + depth, r + TILE_H, h)


def bar(w, h, n_strips):
    """k_connect_cut `dup`: one long run of equal pairs (the ground) broken by a 3-pixel bar that crosses every cut; both keys lie in strip 0 (k_rebase_records, key_add 0 for the survivor)."""
    p = np.full((h, w), GROUND, np.uint8)
    x0 = 100 if w >= 104 else max(0, w // 2 - 1)
    p[:, x0:x0 + 3] = DARK
    return p


def flat(w, h, n_strips, value=GROUND):
    """k_connect_cut `(threadIdx.x & 63) != 0`: one pair repeated across the whole cut, connected once per wave."""
    return np.full((h, w), value, np.uint8)


def stripes(w, h, n_strips):
    """k_connect_cut `pa == a && pb == b`: one-pixel stripes across the cut rows, no two neighbouring lanes carry the same pair -- every lane connects."""
    p = np.full((h, w), GROUND, np.uint8)
    for r, _, _ in cuts(h, n_strips):
        y0, y1 = _band(r, h, 4)
        p[y0:y1, 0::2] = DARK
    return p


def serpent(w, h, n_strips):
    """node_connect under k_connect_cut: ONE dark region whose pieces above the cut (columns 4m .. 4m + 2) meet only through the pieces below it
    (4m + 2 .. 4m + 4) -- a chain of w / 2 same-level unions across one cut."""
    p = np.full((h, w), GROUND, np.uint8)
    x = np.arange(w)
    for r, _, _ in cuts(h, n_strips):
        y0, y1 = _band(r, h, 3)
        p[y0:r, x % 4 != 3] = DARK
        p[r:y1, x % 4 != 1] = DARK
    return p


def u_shape(w, h, n_strips, mirror=False, three=False):
    """k_rebase_records `key_add` / `y_add` and k_reduce over a cut: two arms joined only by a bridge on the other side of the cut (mirror: the bridge,
    and so the key, above and most of the area below; three: the arms run through a whole strip between bridge-less ends)."""
    p = np.full((h, w), GROUND, np.uint8)
    xa, xb = (2, w - 5) if w >= 12 else (0, w - 1)
    aw = 3 if w >= 12 else 1
    cs = cuts(h, n_strips)
    if three:
        assert len(cs) >= 2
        (r1, _, _), (r2, _, _) = cs[0], cs[1]
        y0, _ = _band(r1, h, 6)
        _, y1 = _band(r2, h, 3)
        p[y0:r2, xa:xa + aw] = DARK
        p[y0:r2, xb:xb + aw] = DARK
        p[r2:y1, xa:xb + aw] = DARK
        return p
    for r, _, _ in cs[::2] if len(cs) > 1 else cs:             # every other cut: the shapes of neighbouring cuts must not touch
        if mirror:
            am = max(aw, w // 4)                                # a one-row bridge above, wide arms below
            y1 = _band(r, h, 20)[1]
            p[r - 1:r, xa:xb + aw] = DARK
            p[r:y1, xa:xa + am] = DARK
            p[r:y1, xb + aw - am:xb + aw] = DARK
        else:
            y0, y1 = _band(r, h, 10)[0], _band(r, h, 3)[1]
            p[y0:r, xa:xa + aw] = DARK
            p[y0:r, xb:xb + aw] = DARK
            p[r:y1, xa:xb + aw] = DARK
    return p


def rings(w, h, n_strips, step=8, n_rings=None, wall_ring=None, cut=0):
    """k_connect_cut -> node_connect with unequal levels on both sides: tree_planes.ring_plane centred on a cut, a chain of single children as deep as
    the step allows, every ring cut twice (wall_ring: a sealed inside, NONE entries in the border rows)."""
    if n_rings is None:
        n_rings = 255 // step
    big = tp.ring_plane(n_rings, step, centre=(4, 2), wall_ring=wall_ring)          # 256 x 256, centre pixels at (127 | 128, 127 | 128)
    big = np.pad(big, ((0, 0), (0, 1)), mode="edge")                                # (a 257th column for the widest crop)
    r = cuts(h, n_strips)[cut][0] if cuts(h, n_strips) else h // 2
    y0, x0 = 128 - r, 128 - w // 2                                                  # the centre on the cut, in the middle of the width
    assert 0 <= y0 and y0 + h <= 256 and 0 <= x0 and x0 + w <= 257
    return np.ascontiguousarray(big[y0:y0 + h, x0:x0 + w])


def levels_across(w, h, n_strips, on_64=False, unit=32):
    """node_connect's three cases in a chosen order along one cut: level above < below, ==, > below, the boundaries of the thirds on x = 64 k or off it."""
    if on_64:
        b1, b2 = (64, 256) if w > 256 else (64, 128)
    else:
        b1, b2 = w // 3, 2 * w // 3
    p = np.full((h, w), 3 * unit, np.uint8)
    for r, _, _ in cuts(h, n_strips):
        y0, y1 = _band(r, h, 3)
        p[y0:r, :b1], p[r:y1, :b1] = unit, 2 * unit
        p[y0:r, b1:b2], p[r:y1, b1:b2] = 2 * unit, 2 * unit
        p[y0:r, b2:], p[r:y1, b2:] = 2 * unit, unit
    return p


CORNER_X = {"a": (0, 62, 64), "b": (0, 63)}


def corner_columns(w, variant):
    """The x of the corners of one plane.  x = 62, 63, 64 in ONE plane would put (r - 1, 63) over (r, 63): a pixel pair, not a corner.  So there are two
    planes, a = {0, 62, 64, w - 2} and b = {0, 63, w - 2}, each without an x next to one it holds already."""
    xs = []
    for x in CORNER_X[variant] + (w - 2,):
        if 0 <= x and x + 1 < w and all(abs(x - y) > 1 for y in xs):
            xs.append(x)
    return xs


def corner(w, h, n_strips, variant="a"):
    """k_connect_cut joins (x above, x below) and nothing else: dark pixels at (r - 1, x) and (r, x + 1) only meet at a corner and stay separate regions."""
    p = np.full((h, w), GROUND, np.uint8)
    for r, _, _ in cuts(h, n_strips):
        for x in corner_columns(w, variant):
            p[r - 1, x] = DARK
            p[r, x + 1] = DARK
    return p


def _textured(w, h, n_strips):
    p = np.full((h, w), GROUND, np.uint8)
    for r, _, _ in cuts(h, n_strips):
        y0, y1 = _band(r, h, 6)
        p[y0:y1, 1::5] = MID                       # columns of a lower level through the cut rows on both sides
        p[y0:y1:2, 3::10] = DARK
    return p


def wall_cut(w, h, n_strips, kind="above"):
    """k_strip_border_ids `e == 0xFFFF` / k_connect_cut `a != NONE && b != NONE`: a cut row made of walls.  above: the last row above every cut is sentinel
    (the lower part is sealed off); below: the first row below has walls at x = 0, 63, 64, w - 1 and at every other pixel; both: both rows sentinel."""
    p = _textured(w, h, n_strips)
    for r, _, _ in cuts(h, n_strips):
        if kind in ("above", "both"):
            p[r - 1, :] = WALL
        if kind == "both":
            p[r, :] = WALL
        if kind == "below":
            p[r, 1::2] = WALL
            for x in (0, 63, 64, w - 1):
                if x < w:
                    p[r, x] = WALL
    return p


def empty_strip(w, h, n_strips, which=1):
    """str_er_strip_merge_ex: a strip with rows and no record (n_nodes 0, `if (!p.n_nodes) continue`, top and bot rows all NONE); its complement is one flat region."""
    p = _textured(w, h, n_strips)
    s = cut_rows(h, n_strips)[which]
    assert s.rows > 0 and s.has_top and s.has_bot
    p[s.r0:s.r1] = WALL
    return p


# ---- past one grid round of k_rebase_records / k_check_forest -----------------------------------------------------------------
BIG_TILES_X, BIG_TILE_ROWS, BIG_TILE_NODES = 32, 36, 965


def big_tile():
    """The full checkerboard of speckles (1025 nodes) with an 11 x 11 block of a middle level in it: 965 nodes, above both fold limits of the tile kernel, so
    every node is exported -- and one of them, the block (area > 120), is kept: every tile has a record of its own in the result."""
    t = tp.speckle_tile(1025)
    t[10:21, 20:31] = MID
    return t


def big_strips_plane():
    """k_rebase_records / k_check_forest `i += gridDim.x * blockDim.x`: two strips of 32 x 36 big tiles -- 1 111 680 records > 2^20 in the top strip and as
    many in the bottom one.  Rebasing the top strip's records changes nothing (delta, key_add and y_add are 0); the bottom strip's have to move, and
    whichever tiles got the ids past 2^20, each has its block in the result."""
    return np.tile(big_tile(), (2 * BIG_TILE_ROWS, BIG_TILES_X))


# =================================================================================================================================
# the cases: builder -> [(name, plane, n_strips)]
# =================================================================================================================================
def _sizes(pairs, counts=None, min_cuts=0):
    out = []
    for w, h in pairs:
        for n in (counts(h) if counts else strip_counts(h)):
            if len(cuts(h, n)) >= min_cuts:
                out.append((w, h, n))
    return out


def cases():
    """name -> (plane, n_strips).  Every builder has a width on each side of 64 and of 256; every strip count of strip_counts(h) is on at least two builders
    (bar, flat and serpent take all of them)."""
    out = {}

    def add(kind, w, h, n, plane):
        out["%s/%dx%d/%d" % (kind, w, h, n)] = (plane, n)

    for w, h, n in _sizes([(63, 33), (65, 65), (255, 64), (257, 97)]):
        add("bar", w, h, n, bar(w, h, n))
    for w, h, n in _sizes([(1, 33), (64, 64), (65, 97), (256, 65), (257, 96)]):
        add("flat", w, h, n, flat(w, h, n))
    add("flat0", 65, 65, 3, flat(65, 65, 3, 0))
    for w, h, n in _sizes([(63, 33), (65, 96), (255, 65), (257, 97)], min_cuts=1):
        add("serpent", w, h, n, serpent(w, h, n))
    for w, h, n in _sizes([(63, 65), (64, 33), (256, 64), (257, 97)], lambda h: (2, tile_rows(h), 2 * tile_rows(h) + 1), 1):
        add("stripes", w, h, n, stripes(w, h, n))
    for w, h, n in _sizes([(63, 64), (65, 33), (255, 97), (257, 65)], lambda h: (2, tile_rows(h) + 1), 1):
        add("u", w, h, n, u_shape(w, h, n))
        add("u_mirror", w, h, n, u_shape(w, h, n, mirror=True))
    for w, h, n in ((63, 65, 3), (65, 65, 3), (255, 97, 4), (257, 96, 7)):
        add("u_three", w, h, n, u_shape(w, h, n, three=True))
    for w, h, n in _sizes([(63, 64), (65, 97), (255, 96), (257, 65)], lambda h: (2, tile_rows(h)), 1):
        add("rings8", w, h, n, rings(w, h, n, 8))
        add("rings8_wall20", w, h, n, rings(w, h, n, 8, wall_ring=20))
    for w, h, n in _sizes([(63, 65), (64, 33), (65, 64), (255, 97), (256, 96), (257, 65)], lambda h: (2, tile_rows(h) + 1), 1):
        add("levels", w, h, n, levels_across(w, h, n))
        if w > 128:
            add("levels_on64", w, h, n, levels_across(w, h, n, on_64=True))
    for w, h, n in _sizes([(63, 33), (65, 64), (255, 65), (257, 97)], lambda h: (2, 2 * tile_rows(h) + 1), 1):
        add("corner", w, h, n, corner(w, h, n, "a"))
        add("corner_b", w, h, n, corner(w, h, n, "b"))
    for w, h, n in _sizes([(63, 97), (65, 33), (256, 64), (257, 65)], lambda h: (2, tile_rows(h)), 1):
        for kind in ("above", "below", "both"):
            add("wall_" + kind, w, h, n, wall_cut(w, h, n, kind))
    for w, h, n in ((63, 65, 3), (65, 97, 4), (255, 96, 3), (257, 97, 9)):
        which = 1 if n < 9 else 4
        p = empty_strip(w, h, n, which)
        add("empty", w, h, n, p)
        add("empty_inverted", w, h, n, 255 - p)            # the frame inverted and rebuilt: channel 0 carries the complement, the strip of walls is one flat region of level 0
    return out


STEP_UNIT_KINDS = ("rings", "serpent", "levels", "wall")


def step_cases(step):
    """The planes run at every accepted thresh step: name -> (plane, n_strips).  rings: as many rings as the step has levels below the wall level; the
    others use the values 0 / 64 / 128 (levels 32 apart or more: distinct at every step up to 32) and 255."""
    out = {}
    n = 255 // step
    out["rings/257x97/4"] = (rings(257, 97, 4, step, n, cut=1), 4)
    out["rings/65x64/2"] = (rings(65, 64, 2, step, n), 2)
    if n > 12:
        out["rings_wall/255x65/3"] = (rings(255, 65, 3, step, n, wall_ring=10), 3)
    out["serpent/257x65/3"] = (serpent(257, 65, 3), 3)
    out["serpent/63x33/2"] = (serpent(63, 33, 2), 2)
    out["levels/257x96/3"] = (levels_across(257, 96, 3, on_64=True), 3)
    out["levels/65x33/5"] = (levels_across(65, 33, 5), 5)
    for kind in ("above", "below", "both"):
        out["wall_%s/257x65/3" % kind] = (wall_cut(257, 65, 3, kind), 3)
    return out
