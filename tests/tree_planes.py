"""Planes made up for the limits of the tile-tree and tile-joining kernels, and a CPU census that says which side of a limit a plane is on.

The tree half of the census (nodes, levels, exported records, records per group) is derived from the definition of the component tree alone, not from
the kernels' code: it quantises the plane as the reference does (rint_half_even(p * float32(1 / step)), walls at 255 // step + 1), cuts it into
64 x 32 tiles and, tile by tile, labels {level <= t} with scipy for every level t present.  What it reports is what the kernels' limits are stated
in (er_tile_tree.inl, tile2_body.h, er_tree_passes.inl):

  nodes     per tile: the components of {L <= t} that hold a level-t pixel, over all t;
  levels    per tile: the distinct non-wall levels;
  exported  per tile, by the rule both tile kernels implement while a tile folds its closed nodes: a node leaves the tile when its component lies on
            a tile side that has a neighbouring tile, when its area (pixels + nodes of its subtree) exceeds MIN_AREA, when it has no parent inside
            the tile, or when it is the node of the flood's start pixel.  A tile with more nodes than the kernel's fold limit exports every node;
  records   per group of GX x GY tiles: the sum over the group's tiles.

The k_tile_tree2 half is NOT independent of the kernel: `pair_levels` (the wall level of thresh step 8 read as level 0), the per-level count of
the nodes its bulk path does not take (single-row runs off the open sides in a row with at most MIN_AREA / 2 pixels so far, in a tile without
walls that is not half A of the start tile) and `pair_steps` restate conditions of tile2_body.h, because "levels" and "node steps" are defined by
that code and by nothing else.  `tile2_outcome` predicts from them which tiles of a pair the kernel hands back (more than 12 levels in the pair,
more than 160 node steps, more than 64 exported records in a tile); tests/test_tree_edges.py checks the prediction against the kernel's own
source run on the host (tests/cpp/tile2_model_check.cpp) before any GPU test relies on it.  `seam_blocks` likewise restates the host's table of
k_seam workgroups (upload_layout in str_er_api.cpp).

The builders return uint8 planes; every test that uses one asserts with the census that it reaches the line it was made for.
"""
import numpy as np
from scipy import ndimage

TILE_W, TILE_H = 64, 32
SPARSE_FOLD = 332            # k_tile_tree<480>: folds iff 5 * n_even <= 1664
DENSE_FOLD = 880             # k_tile_tree<880>: folds iff n <= 880
SPARSE_CHUNK, DENSE_CHUNK = 480, 512      # nodes per pass of the export-everything path
DENSE_LIST_WORDS = 3520      # 4 * 880: the export list is kept in LDS iff 4 * n_even + exported <= 3520
T2_LEVELS, T2_RECORDS, T2_STEPS = 12, 64, 160
GROUP_TABLES = {0: 512, 4: 2048, 6: 2528}       # STR_ER_GROUP_KERNEL variant -> records of the LDS table
SEAM_BLOCK = 512
UNDONE_GRID = 2048


def quantise(plane, step):
    """Levels of a plane and the wall level."""
    q = np.rint(plane.astype(np.float32) * np.float32(1.0 / step)).astype(np.int32)
    return q, 255 // step + 1


class Tile:
    __slots__ = ("nodes", "levels", "fold_exported", "nonbulk", "walls", "outside", "start")

    def exported(self, fold_cap):
        return self.fold_exported if self.nodes <= fold_cap else self.nodes


def _tile(L, wall, sides, start, min_area, outside):
    """One tile: L levels, wall mask, sides = (top, bottom, left, right) have a neighbouring tile, start = the flood's start pixel or None."""
    h, w = L.shape
    t_ = Tile()
    t_.walls = bool(wall.any())
    t_.outside = outside
    t_.start = start is not None
    levels = np.unique(L[~wall])
    t_.levels = set(int(x) for x in levels)
    side_px = np.zeros((h, w), bool)
    if sides[0]: side_px[0, :] = True
    if sides[1] and h == TILE_H: side_px[-1, :] = True
    if sides[2]: side_px[:, 0] = True
    if sides[3] and w == TILE_W: side_px[:, -1] = True
    marks = np.zeros(h * w, np.int64)
    bulk_ok = not t_.walls and not outside and not t_.start and h >= 2
    nodes = exported = 0
    t_.nonbulk = {}
    for t in levels:
        M = (L <= t) & ~wall
        lab, n = ndimage.label(M)
        flat = lab.ravel()
        own = np.flatnonzero(((L == t) & ~wall).ravel())
        ids, first = np.unique(flat[own], return_index=True)
        marks[own[first]] += 1                      # a node's key pixel: its first own-level pixel in raster order
        pix = np.bincount(flat, minlength=n + 1)[ids]
        nod = np.bincount(flat, weights=marks, minlength=n + 1)[ids]
        is_open = np.bincount(flat, weights=side_px.ravel(), minlength=n + 1)[ids] > 0
        above = ~M & ~wall                          # flooded pixels of a higher level: a component next to one has a parent in the tile
        nb = np.zeros((h, w), bool)
        nb[:-1] |= above[1:]; nb[1:] |= above[:-1]; nb[:, :-1] |= above[:, 1:]; nb[:, 1:] |= above[:, :-1]
        has_parent = np.bincount(flat, weights=(nb & M).ravel(), minlength=n + 1)[ids] > 0
        is_start = np.zeros(len(ids), bool)
        if start is not None and L[start] == t:
            is_start = ids == lab[start]
        exp = is_open | (pix + nod > min_area) | ~has_parent | is_start
        nodes += len(ids)
        exported += int(exp.sum())
        # k_tile_tree2's bulk path: the node is one run of its row with nothing of M above or below, off the open sides, in a row that holds at most
        # MIN_AREA / 2 pixels of M
        objs = ndimage.find_objects(lab)
        rowpix = M.sum(axis=1)
        nb_count = 0
        for i, o in zip(ids, is_open):
            sl = objs[i - 1]
            one_row = sl[0].stop - sl[0].start == 1
            if not (bulk_ok and one_row and not o and 2 * int(rowpix[sl[0].start]) <= min_area):
                nb_count += 1
        t_.nonbulk[int(t)] = nb_count
    t_.nodes, t_.fold_exported = nodes, exported
    return t_


class Census:
    """Tile by tile census of one plane."""

    def __init__(self, plane, step=8, min_area=120):
        plane = np.asarray(plane, np.uint8)
        self.h, self.w = plane.shape
        self.step, self.min_area = step, min_area
        q, self.hi = quantise(plane, step)
        wall = q >= self.hi
        self.n_walls = int(wall.sum())
        self.tiles_x, self.tiles_y = -(-self.w // TILE_W), -(-self.h // TILE_H)
        start = None
        if not wall[0, 0]: start = (0, 0)
        elif self.w > 1 and not wall[0, 1]: start = (0, 1)
        elif self.h > 1 and not wall[1, 0]: start = (1, 0)
        self.tiles = {}
        for ty in range(self.tiles_y):
            for tx in range(self.tiles_x):
                ys, xs = slice(ty * TILE_H, (ty + 1) * TILE_H), slice(tx * TILE_W, (tx + 1) * TILE_W)
                L = q[ys, xs]
                outside = L.shape != (TILE_H, TILE_W)
                self.tiles[ty, tx] = _tile(L, wall[ys, xs], (ty > 0, ty + 1 < self.tiles_y, tx > 0, tx + 1 < self.tiles_x),
                                           start if (ty, tx) == (0, 0) else None, min_area, outside)

    def nodes(self):
        return np.array([[self.tiles[y, x].nodes for x in range(self.tiles_x)] for y in range(self.tiles_y)])

    def exported(self, fold_cap):
        return np.array([[self.tiles[y, x].exported(fold_cap) for x in range(self.tiles_x)] for y in range(self.tiles_y)])

    def records(self, fold_cap):
        return int(self.exported(fold_cap).sum())

    def group_records(self, gx, gy, fold_cap):
        e = self.exported(fold_cap)
        return np.array([[int(e[y:y + gy, x:x + gx].sum()) for x in range(0, self.tiles_x, gx)] for y in range(0, self.tiles_y, gy)])

    # ---- k_tile_tree2 ----
    def pair_levels(self, ty, tx):
        """Levels k_tile_tree2 counts for the pair (tx, tx + 1), tx even.  Beyond the distinct non-wall levels of the two tiles: the kernel finds the
        levels with a shift by (level & 31), so at thresh step 8 (wall level 32) a wall, a pixel outside the image or a missing tile B reads as
        level 0 -- one level more unless level 0 is there anyway."""
        a, b = self.tiles[ty, tx], self.tiles.get((ty, tx + 1))
        lv = set(a.levels) | (set(b.levels) if b else set())
        if self.hi == 32 and (b is None or a.walls or a.outside or b.walls or b.outside):
            lv.add(0)
        return lv

    def pair_steps(self, ty, tx):
        a, b = self.tiles[ty, tx], self.tiles.get((ty, tx + 1))
        nb = b.nonbulk if b else {}
        return sum(max(a.nonbulk.get(t, 0), nb.get(t, 0)) for t in set(a.nonbulk) | set(nb))

    def tile2_taken(self):
        return self.hi <= 32 and self.hi >= 2 and self.step & (self.step - 1) == 0

    def tile2_outcome(self):
        """(tiles given to k_tile_tree2, set of (ty, tx) it hands back).  Raises where two limits are crossed in one pair (the order in which the
        kernel meets them would matter)."""
        if not self.tile2_taken():
            return 0, set()
        back = set()
        for ty in range(self.tiles_y):
            for tx in range(0, self.tiles_x, 2):
                live = [(ty, x) for x in (tx, tx + 1) if (ty, x) in self.tiles]
                if len(self.pair_levels(ty, tx)) > T2_LEVELS:
                    back.update(live)
                    continue
                over = [k for k in live if self.tiles[k].fold_exported > T2_RECORDS]
                steps = self.pair_steps(ty, tx)
                if steps > T2_STEPS:
                    if over:
                        raise AssertionError("pair (%d, %d) crosses the step and the record limit" % (ty, tx))
                    back.update(live)
                else:
                    back.update(over)
        return self.tiles_x * self.tiles_y, back

    def tile2_records(self):
        """Records of the plane when every tile goes to k_tile_tree2 first (the tiles it hands back are the small k_tile_tree's)."""
        _, back = self.tile2_outcome()
        return sum(t.exported(SPARSE_FOLD) if k in back else t.fold_exported for k, t in self.tiles.items())


def seam_blocks(w, h, gx, gy):
    """(first pair of every k_seam workgroup, n_hpairs, n_pairs) of a w x h plane with groups of gx x gy tiles (0, 0: no groups) -- the table
    upload_layout (str_er_api.cpp) makes: pairs are numbered seam by seam, the horizontal seams first (w pairs each), then the vertical ones (h
    each); a workgroup takes SEAM_BLOCK consecutive pairs.  Without groups the blocks run through all pairs from 0; with groups every seam
    BETWEEN groups starts a block list of its own, and its last block reaches into the pairs behind the seam."""
    tx, ty = -(-w // TILE_W), -(-h // TILE_H)
    n_h = w * (ty - 1)
    n = n_h + h * (tx - 1)
    if gx > 0 and gy > 0:
        firsts = []
        for j in range(gy - 1, ty - 1, gy):
            firsts += list(range(j * w, (j + 1) * w, SEAM_BLOCK))
        for k in range(gx - 1, tx - 1, gx):
            firsts += list(range(n_h + k * h, n_h + (k + 1) * h, SEAM_BLOCK))
    else:
        firsts = list(range(0, n, SEAM_BLOCK))
    return firsts, n_h, n


# =================================================================================================================================
# builders
# =================================================================================================================================
BG = 128                     # background of the speckle planes: level 16 at step 8, 8 at step 16


def _cells(interior=True):
    """Cells of a 64 x 32 tile no two of which are 4-neighbours, in a fixed order: the inner checkerboard first (930 cells), then the border's."""
    inner, border = [], []
    for r in range(TILE_H):
        for c in range(TILE_W):
            if (r + c) % 2 == 0:
                (inner if 0 < r < TILE_H - 1 and 0 < c < TILE_W - 1 else border).append((r, c))
    return inner if interior else inner + border


def speckle_tile(n_nodes, bg=BG, fg=0):
    """A 64 x 32 tile with exactly n_nodes nodes: n_nodes - 1 isolated pixels of a lower level on a flat background.  Up to 931 nodes the speckles stay
    off the tile's border cells (closed nodes of area 2); up to 1025 they fill the checkerboard."""
    k = n_nodes - 1
    cells = _cells(k <= 930)
    assert 0 <= k <= len(cells)
    t = np.full((TILE_H, TILE_W), bg, np.uint8)
    for r, c in cells[:k]:
        t[r, c] = fg
    return t


def vspeckle_tile(n_nodes, bg=BG, fg=0):
    """n_nodes - 1 closed two-pixel VERTICAL speckles (rows 3j + 1, 3j + 2, every other column) on a flat background: not single-row runs, so
    k_tile_tree2 takes a node step for each."""
    t = np.full((TILE_H, TILE_W), bg, np.uint8)
    cells = [(r, c) for r in range(1, TILE_H - 2, 3) for c in range(1, TILE_W - 1, 2)]
    assert n_nodes - 1 <= len(cells)
    for r, c in cells[:n_nodes - 1]:
        t[r:r + 2, c] = fg
    return t


def graded_tile(seed=0):
    """More nodes than pixels / 2 (thresh step 1): a checkerboard of level-0 minima, the other cells at scattered levels 1 .. 255."""
    rng = np.random.default_rng(seed)
    t = rng.integers(1, 256, (TILE_H, TILE_W)).astype(np.uint8)
    rr, cc = np.indices(t.shape)
    t[(rr + cc) % 2 == 0] = 0
    return t


def place(w, h, tiles, bg=BG):
    """A w x h plane of `bg` with the given 64 x 32 tiles at their (ty, tx), cut at the plane's edge."""
    p = np.full((h, w), bg, np.uint8)
    for (ty, tx), t in tiles.items():
        y, x = ty * TILE_H, tx * TILE_W
        p[y:y + TILE_H, x:x + TILE_W] = t[:min(TILE_H, h - y), :min(TILE_W, w - x)]
    return p


def positions_plane(tile, bg=BG):
    """3 x 3 tiles: `tile` as the plane's first tile (it holds the start pixel), as an interior tile and as the last one."""
    return place(3 * TILE_W, 3 * TILE_H, {(0, 0): tile, (1, 1): tile, (2, 2): tile}, bg)


def ragged_plane(tile, w, h, bg=BG):
    """`tile` whole as the first tile of a w x h plane (64 < w < 128, 32 < h < 64) whose other three tiles are ragged; the last one holds a few speckles."""
    p = place(w, h, {(0, 0): tile}, bg)
    for r, c in ((TILE_H + 0, TILE_W), (h - 1, w - 1), (TILE_H + 2, w - 1)):
        if r < h and c < w:
            p[r, c] = 0
    return p


def tile_family(counts):
    """The planes of one tile kernel's node-count limits, (name, plane, nodes): every count at the three positions and with ragged neighbours."""
    out = []
    for n in counts:
        t = speckle_tile(n)
        out.append(("n%d/positions" % n, positions_plane(t), n))
        out.append(("n%d/127x63" % n, ragged_plane(t, 127, 63), n))
        out.append(("n%d/65x33" % n, ragged_plane(t, 65, 33), n))
    return out


SPARSE_COUNTS = (255, 256, 257, 331, 332, 333, 334, 480, 481, 960, 961)
DENSE_COUNTS = (879, 880, 881, 882, 1024, 1025)
LISTED_COUNTS = (704, 705)


# ---- thresh steps 1 and 2 ----
def pair_plane(step):
    """Vertical and horizontal neighbour pairs at the levels where the per-column loop's 8-bit weights could wrap or collide with its wall marker,
    one pair per tile of a 4 x 2-tile plane and one pair across each seam."""
    vals = ((126, 127), (127, 128), (128, 129), (254, 255)) if step == 1 else ((252, 253), (253, 254), (254, 255), (250, 255))
    p = np.full((2 * TILE_H, 4 * TILE_W), 60, np.uint8)
    for i, (a, b) in enumerate(vals):
        x = i * TILE_W
        p[5, x + 10], p[6, x + 10] = a, b                    # vertical pair
        p[12, x + 20], p[12, x + 21] = b, a                  # horizontal pair
        p[TILE_H - 1, x + 30], p[TILE_H, x + 30] = a, b      # across the horizontal seam
        p[TILE_H + 9, x + 40], p[TILE_H + 10, x + 40] = b, a
        p[20, x + 7:x + 9] = (a, b)                          # inside one lane's 8 pixels
    for i, (a, b) in enumerate(vals[:3]):
        p[25, (i + 1) * TILE_W - 1], p[25, (i + 1) * TILE_W] = a, b      # across the vertical seams
    return p


def staircase_plane():
    """All 256 levels of thresh step 1 inside one group of tiles (2 x 2 tiles): every tile holds 64 levels, one a column, the four tiles of the group
    hold 0 .. 255 between them."""
    p = np.zeros((2 * TILE_H, 2 * TILE_W), np.uint8)
    for ty in range(2):
        for tx in range(2):
            base = 128 * ty + 64 * tx
            p[ty * TILE_H:(ty + 1) * TILE_H, tx * TILE_W:(tx + 1) * TILE_W] = (base + np.arange(TILE_W))[None, :]
    return p


# ---- k_tile_tree2 ----
def level_tile(values):
    """Vertical bands of the given pixel values, 4 columns each, the last one filling the tile."""
    t = np.full((TILE_H, TILE_W), values[-1], np.uint8)
    for i, v in enumerate(values[:-1]):
        t[:, 4 * i:4 * i + 4] = v
    return t


def levels(step, n, first=0):
    """n pixel values of n consecutive levels at a power-of-two thresh step."""
    return [step * (first + i) for i in range(n)]


def record_tile(n_records, bg=BG):
    """A tile with exactly n_records exported nodes at MIN_AREA 120 where all four of its sides have a neighbouring tile: the background and
    n_records - 1 single dark pixels on its border (open nodes), no two of them neighbours."""
    t = np.full((TILE_H, TILE_W), bg, np.uint8)
    spots = [(r, c) for r in (0, TILE_H - 1) for c in range(1, TILE_W - 1, 2)] + [(r, c) for c in (0, TILE_W - 1) for r in range(2, TILE_H - 2, 2)]
    assert n_records - 1 <= len(spots)
    for r, c in spots[:n_records - 1]:
        t[r, c] = 0
    return t


# ---- k_group_merge ----
def group_plane(tiles_x, tiles_y, counts, bg=BG):
    """tiles_x x tiles_y tiles, tile (ty, tx) a speckle tile with counts[ty][tx] nodes (0: a tile of walls)."""
    p = np.full((tiles_y * TILE_H, tiles_x * TILE_W), bg, np.uint8)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            n = counts[ty][tx]
            t = np.full((TILE_H, TILE_W), 255, np.uint8) if n == 0 else speckle_tile(n, bg)
            p[ty * TILE_H:(ty + 1) * TILE_H, tx * TILE_W:(tx + 1) * TILE_W] = t
    return p


def cap_plane(gx, gy, cap, extra, groups_x=3, groups_y=1, bg=BG):
    """groups_x x groups_y groups of gx x gy tiles at MIN_AREA 1 (every node is a record): the middle group holds exactly cap + extra nodes, the
    others a fifth of that."""
    nt = gx * gy
    counts = [[max(1, cap // (5 * nt))] * (gx * groups_x) for _ in range(gy * groups_y)]
    mid_x, mid_y = (groups_x // 2) * gx, (groups_y // 2) * gy
    total = cap + extra
    per = total // nt
    for i in range(nt):
        counts[mid_y + i // gx][mid_x + i % gx] = per + (1 if i < total - per * nt else 0)
    return group_plane(gx * groups_x, gy * groups_y, counts, bg)


# ---- seams ----
def lattice_plane(w=1024, h=832, per_tile=400, bg=BG):
    """`per_tile` closed speckles in every (whole) tile."""
    t = speckle_tile(per_tile + 1, bg)
    return np.tile(t, (-(-h // TILE_H), -(-w // TILE_W)))[:h, :w].copy()


def ring_plane(n_rings, step, centre, wall_ring=None):
    """Square rings of rising level around the corner that tiles (cty - 1 | cty, ctx - 1 | ctx) share, centre = (cty, ctx): a chain of single children as
    deep as there are rings, every ring cut by all four seams.  wall_ring: that ring is made of walls -- what lies inside is sealed off from the start pixel."""
    cy, cx = centre[0] * TILE_H, centre[1] * TILE_W
    assert n_rings < min(cy, cx) and n_rings * step <= 255 and n_rings < 255 // step + 1
    yy, xx = np.indices((2 * cy, 2 * cx))
    d = np.maximum(np.where(yy < cy, cy - 1 - yy, yy - cy), np.where(xx < cx, cx - 1 - xx, xx - cx))       # 0 at the four centre pixels
    p = (np.minimum(d, n_rings) * step).astype(np.uint8)
    if wall_ring is not None:
        p[d == wall_ring] = 255
    return p


def interleaved_staircases(vertical_seam=True):
    """Two staircases of 125 levels each at thresh step 1, one with the even and one with the odd levels, meeting across a seam: joining them is a merge
    250 levels deep."""
    n = 125
    if vertical_seam:
        p = np.zeros((TILE_H, 4 * TILE_W), np.uint8)
        for i in range(n):
            p[:, 2 * TILE_W - 1 - i] = 2 * i                  # left of the seam: even levels rising away from it
            p[:, 2 * TILE_W + i] = 2 * i + 1                  # right: odd levels
        p[:, :2 * TILE_W - n] = 250
        p[:, 2 * TILE_W + n:] = 251
        return p
    p = np.zeros((8 * TILE_H, TILE_W), np.uint8)
    for i in range(n):
        p[4 * TILE_H - 1 - i, :] = 2 * i
        p[4 * TILE_H + i, :] = 2 * i + 1
    p[:4 * TILE_H - n, :] = 250
    p[4 * TILE_H + n:, :] = 251
    return p


def columns_plane():
    """Columns 0 .. 63 ascending in every tile (thresh step 1), two tile rows of eight tiles: the 512 pixel pairs of the horizontal seam are 512 different
    pairs of nodes."""
    return np.tile(np.arange(TILE_W, dtype=np.uint8)[None, :] * 3, (2 * TILE_H, 8))


def stripes_plane(n, vertical=False):
    """Two tile rows, n wide: background | dark column | background ... crossing the seam -- two pairs of nodes alternating along it.  vertical: two
    tile columns, n high, dark rows crossing the vertical seam."""
    if vertical:
        p = np.full((n, 2 * TILE_W), BG, np.uint8)
        p[1::2, TILE_W - 3:TILE_W + 3] = 0
        return p
    p = np.full((2 * TILE_H, n), BG, np.uint8)
    p[TILE_H - 3:TILE_H + 3, 1::2] = 0
    return p


# ---- the global passes ----
def many_children_plane(tiles=9):
    """One parent (the background) with more than 4096 open children: two-pixel dark speckles straddling every seam of tiles x tiles tiles."""
    s = tiles
    p = np.full((s * TILE_H, s * TILE_W), BG, np.uint8)
    for j in range(1, s):
        p[j * TILE_H - 1:j * TILE_H + 1, 1:-1:2] = 0          # across horizontal seams
    for i in range(1, s):
        rows = [r for r in range(2, s * TILE_H - 2, 2) if r % TILE_H not in (0, 1, TILE_H - 1, TILE_H - 2)]
        p[rows, i * TILE_W - 1] = 0
        p[rows, i * TILE_W] = 0
    return p


def pushing_children_plane():
    """Blobs (level 8 at step 8) centred on the vertical seams of a 6 x 2-tile plane; blob k holds k = 1 .. 5 darker sub-blobs (level 2) that cross the
    seam themselves: parents with exactly 1 .. 5 children that are still open when the tiles are joined."""
    p = np.full((2 * TILE_H, 6 * TILE_W), BG, np.uint8)
    for k in range(1, 6):
        x = k * TILE_W
        p[4:4 + 4 * k + 1, x - 6:x + 6] = 64
        for j in range(k):
            p[5 + 4 * j:5 + 4 * j + 2, x - 3:x + 3] = 16
    return p
