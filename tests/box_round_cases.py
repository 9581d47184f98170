"""The inputs and the expected outputs of test_box_rounds.py (the kernels) and test_box_round_cases.py (the premises, no GPU): batches
of more boxes than a capped grid has workgroups, so that every workgroup of a per-box kernel walks on to a second box and a few to a
third.  Not a test module.

A batch is K distinct hand-made cases repeated cyclically to N boxes.  K is odd, so it does not divide the grid: the boxes a
workgroup takes in successive rounds (i, i + GRID_CAP, ...) are different cases, and what the first left in LDS is not what the
second needs.  Every reference (the flood, shape_ref, stroke_ref, line_geom_ref, line_words_ref, the numpy sampler of the crops) runs
on the K cases alone; `extend` repeats its result to N boxes and cumulative sums give the offsets, so nothing here loops over N.
The references are computed once per process and shared by both modules."""
import functools

import numpy as np

import line_geom_ref as LG
import line_words_ref as LW
import test_line_crops_abi as CROP
from shape_ref import shape_ref
from stroke_ref import stroke_ref
from test_er_masks import _rings, flood, pack

# The cap of the grids, as the launches have it:
#   er_masks.inl       launch_er_masks_t:                      const int grid_cap = 1 << 16;
#   er_frame_lines.inl launch_foot_geom, launch_foot_words:    const dim3 grid((unsigned)std::min(n_lines, 1 << 16));
#   er_line_crops.inl  launch_line_crops:                      const dim3 grid((unsigned)std::min(n, 1 << 16));
GRID_CAP = 65536
K = 9                               # cases a cycle
N = 2 * GRID_CAP + 5                # boxes a launch: every workgroup takes a second box, five take a third


def extend(parts, n=N):
    """The per-case arrays `parts` (one per case, joined along axis 0) repeated cyclically to n boxes."""
    parts = [np.asarray(p) for p in parts]
    q, r = divmod(n, len(parts))
    cycle = np.concatenate(parts)
    return np.concatenate([np.tile(cycle, (q,) + (1,) * (cycle.ndim - 1))] + parts[:r])


def starts(counts, n=N):
    """(per-box counts, the index of every box's first element) of per-case element counts, back to back over n boxes."""
    c = extend([[int(v)] for v in counts], n).astype(np.int64)
    return c, np.cumsum(c) - c


def mask_class(w, h):               # er_masks.inl: mask_class
    if w <= 64 and h <= 64:
        return 0
    return 1 if h * ((w + 63) // 64) <= 1024 else 2


# ---- the mask family: er_masks, er_shapes, er_strokes -----------------------------------------------------------------------------------
# One plane, K boxes of the small class and K of the LDS class, a call's regions in the order small 0, LDS 0, small 1, LDS 1, ...: the
# host sorts them by class, so each of the two launches gets N boxes.  The scratch class is left out: it keeps nothing in LDS between
# rounds (A and R are the box's own words of global scratch), and 65537 boxes of more than 1024 words each need about 1 GB of it.
MASK_W, MASK_H = 200, 80
STEP = 8
LUT = np.rint(np.arange(256, dtype=np.float32) * np.float32(1.0 / STEP)).astype(np.int64)      # the quantiser at thresh_step 8
LDS_SIZES = ((65, 1), (130, 2), (96, 3), (129, 4), (100, 4), (128, 5), (70, 5), (127, 2), (66, 16))     # word pitch 2, 3, 2, 3, 2, 2, 2, 2, 2
MASK_WORDS_MAX = 150                # mask words (h * ceil(w / 32)) a cycle of one class: the bindings reserve them per box


def _small_masks():
    """(x, y, bits, key x, key y) of the K small boxes; bits: the pixels at level 0.  Rows 65.. of the plane hold all but the first."""
    one = lambda h, w: np.ones((h, w), bool)                                    # noqa: E731
    ring = one(5, 5); ring[1:4, 1:4] = False                                    # a ring: one hole of 9 pixels
    block = one(4, 4); block[1, 1] = block[2, 2] = False                        # two hole pixels that touch diagonally: one hole
    pair = np.array([[1, 1, 0], [0, 0, 1]], bool)                               # a diagonal pair: the flood from (0, 0) stops short of (2, 1)
    row = one(1, 40); row[0, 17:20] = False                                     # the key's run ends at a gap: row extent 0 .. 17 of 40
    ell = np.zeros((3, 5), bool); ell[:, 0] = ell[2, :] = True
    return [(0, 0, _rings(64) == 0, 0, 0), (0, 65, ring, 0, 0), (7, 65, block, 0, 0), (13, 65, pair, 0, 0), (18, 65, one(1, 1), 0, 0),
            (21, 65, row, 0, 0), (63, 65, one(3, 1), 0, 1), (66, 65, ell, 0, 0), (73, 65, one(1, 33), 32, 0)]


def _lds_masks():
    """(x, y, bits, key x, key y) of the K LDS boxes, stacked at x = 66 with a wall row between them: ragged ink around a joining
    row, so the runs cross the word borders at columns 64 and 128 of the box and the flood has work to do."""
    rng = np.random.default_rng(65536)
    out, y = [], 0
    for w, h in LDS_SIZES:
        bits = rng.random((h, w)) < 0.75
        if h == 1:
            bits[:] = True
            bits[0, 30] = False                                                 # the key's run: columns 31 .. 64, across the word border
            kx, ky = 40, 0
        else:
            bits[h // 2, :] = True
            kx, ky = 0, h // 2
        out.append((66, y, bits, kx, ky))
        y += h + 1
    return out


@functools.lru_cache(maxsize=None)
def mask_cases():
    """(plane, boxes): the (MASK_H, MASK_W) uint8 plane and the 2 K regions of one cycle as (x, y, w, h, key, level), small and LDS
    in turn.  Ink has the grey values 0 .. 3 (level 0 at thresh_step 8), everything else is 255."""
    ink = np.zeros((MASK_H, MASK_W), bool)
    boxes = []
    for small, lds in zip(_small_masks(), _lds_masks()):
        for x, y, bits, kx, ky in (small, lds):
            h, w = bits.shape
            assert not ink[y:y + h, x:x + w].any() and y + h <= MASK_H and x + w <= MASK_W
            ink[y:y + h, x:x + w] = bits
            boxes.append((x, y, w, h, (y + ky) * MASK_W + x + kx, 0))
    yy, xx = np.mgrid[0:MASK_H, 0:MASK_W]
    plane = np.where(ink, (7 * xx + 3 * yy) % 4, 255).astype(np.uint8)
    return plane, boxes


@functools.lru_cache(maxsize=None)
def mask_refs():
    """Per region of the cycle: (mask words, pixels, shape_ref's dict, stroke_ref's dict), by the references of test_er_masks.py,
    test_er_shapes.py and test_er_strokes.py."""
    plane, boxes = mask_cases()
    q = LUT[plane]
    out = []
    for x, y, w, h, key, level in boxes:
        m = flood(q, x, y, w, h, key, level)
        ys, xs = np.nonzero(m)
        out.append((pack(m), int(m.sum()), shape_ref(m, plane[y:y + h, x:x + w]), stroke_ref(m[ys.min():ys.max() + 1, xs.min():xs.max() + 1])))
    return out


def _pairs(per_region):
    """2 K per-region arrays as K parts of one (small, LDS) pair each: a part is a case of `extend`."""
    return [np.concatenate([np.atleast_1d(per_region[2 * k]), np.atleast_1d(per_region[2 * k + 1])]) for k in range(K)]


def mask_regions(n=N):
    """The fields of the 2 n regions of a call: {name: array}."""
    _, boxes = mask_cases()
    return {name: extend(_pairs([[b[i]] for b in boxes]), n) for i, name in enumerate(("x", "y", "w", "h", "key", "level"))}


def mask_expected(n=N):
    """(words, pixels) of er_masks on the 2 n regions."""
    refs = mask_refs()
    return extend(_pairs([r[0] for r in refs]), n), extend(_pairs([[r[1]] for r in refs]), n)


def shape_expected(n=N):
    """{field: array over the 2 n regions} of er_shapes (crossings: (2 n, 4))."""
    refs = mask_refs()
    return {k: extend(_pairs([np.asarray([r[2][k]]) for r in refs]), n) for k in refs[0][2]}


def stroke_expected(n=N):
    refs = mask_refs()
    return {k: extend(_pairs([[r[3][k]] for r in refs]), n) for k in refs[0][3]}


# ---- the footprint kernels: feet_geom, feet_words ------------------------------------------------------------------------------------------
FRAME_W, FRAME_H = 1400, 1200
GEOM_POINTS_MAX = 200               # sum over a cycle of 2 (h + 1): the hull vertices feet_geom reserves
WORD_RUNS_MAX = 140                 # sum over a cycle of (w + 1) // 2: the run and word records feet_words reserves


@functools.lru_cache(maxsize=None)
def geom_cases():
    """K footprints (x, y, bits) with tight boxes, heights 1 .. 30 and different hulls."""
    one = lambda h, w: np.ones((h, w), bool)                                    # noqa: E731
    tri = np.tril(one(30, 30))
    ell = np.zeros((12, 9), bool); ell[:, 0] = ell[11, :] = True
    yy, xx = np.mgrid[-4:5, -4:5]
    slant = np.zeros((20, 14), bool)
    for r in range(20):
        slant[r, r // 2:r // 2 + 5] = True
    two = np.zeros((5, 70), bool)                                               # empty rows inside, rows with bits in the second word only
    two[0, :] = True; two[1, 66:] = True; two[4, :6] = True
    return [(3, 2, one(1, 1)), (31, 5, one(1, 65)), (200, 20, tri), (300, 100, ell), (50, 300, one(3, 40)), (500, 300, abs(xx) + abs(yy) <= 4),
            (700, 400, slant), (33, 40, two), (FRAME_W - 8, FRAME_H - 8, np.eye(8, dtype=bool))]


@functools.lru_cache(maxsize=None)
def words_cases():
    """K footprints (x, y, bits) with tight boxes: one of 130 columns with a run across the word border at column 64, the others of
    at most 16 columns with 1 .. 8 runs; ragged columns, so the runs differ in pixels and row extents."""
    rng = np.random.default_rng(131077)

    def cols(x, y, w, h, cs):
        b = np.zeros((h, w), bool)
        for c in cs:
            rows = rng.random(h) < 0.6
            rows[rng.integers(h)] = True
            b[rows, c] = True
        b[0, 0] = b[h - 1, w - 1] = True
        assert cs[0] == 0 and cs[-1] == w - 1
        return x, y, b

    wide = [0, 1, 2] + list(range(60, 70)) + [100, 127, 128, 129]
    return [cols(7, 11, 130, 3, wide), cols(400, 30, 16, 4, list(range(0, 16, 2)) + [15]), cols(450, 31, 15, 3, list(range(0, 15, 2))),
            cols(500, 32, 13, 7, [0, 1, 2, 3, 5, 6, 9, 10, 11, 12]), cols(550, 33, 11, 2, list(range(11))), cols(600, 34, 9, 5, [0, 1, 4, 5, 6, 7, 8]),
            cols(650, 35, 9, 6, list(range(0, 9, 2))), cols(700, 36, 12, 8, list(range(0, 12, 2)) + [11]), cols(FRAME_W - 1, FRAME_H - 9, 1, 9, [0])]


def feet_args(cases, n=N):
    """({field: array over n footprints} of the foot records, the footprints' words back to back) of K cases (x, y, bits)."""
    rec = {"x": [c[0] for c in cases], "y": [c[1] for c in cases], "w": [c[2].shape[1] for c in cases], "h": [c[2].shape[0] for c in cases],
           "pixels": [int(c[2].sum()) for c in cases]}
    return {k: extend([[v] for v in vs], n) for k, vs in rec.items()}, extend([pack(c[2]) for c in cases], n)


@functools.lru_cache(maxsize=None)
def geom_refs():
    return [LG.geom(b, x, y) for x, y, b in geom_cases()]


def geom_expected(n=N):
    """({field: array over n footprints} of the geometry records, qx and qy as (n, 4), the (points, 2) hull vertices)."""
    refs = geom_refs()
    out = {k: extend([[r[0][k]] for r in refs], n) for k in LG.FIELDS}
    out["count"], out["first"] = starts([len(r[3]) for r in refs], n)
    out["qx"] = extend([[r[1]] for r in refs], n)
    out["qy"] = extend([[r[2]] for r in refs], n)
    return out, extend([np.asarray(r[3], np.int64).reshape(-1, 2) for r in refs], n)


@functools.lru_cache(maxsize=None)
def words_refs():
    """Per case, as a line of its own: (colmax, runs (x0, x1, y0, y1, pixels), words, the word of every run)."""
    out = []
    for x, y, b in words_cases():
        colmax, runs = LW.runs_of(b, x, y)
        words, idx = LW.words_of(runs, colmax)
        out.append((colmax, runs, words, idx))
    return out


def words_expected(n=N):
    """The three tables of feet_words on n footprints at the gap 1 / 3, each {field: array}: line_words, runs, words."""
    refs = words_refs()
    n_runs, first_run = starts([len(r[1]) for r in refs], n)
    n_words, first_word = starts([len(r[2]) for r in refs], n)
    lines = {"first_word": first_word, "n_words": n_words, "first_run": first_run, "n_runs": n_runs, "colmax": extend([[r[0]] for r in refs], n),
             "reserved": np.zeros(n, np.int64)}
    run_t = extend([np.asarray(r[1], np.int64).reshape(-1, 5) for r in refs], n)
    runs = {k: run_t[:, i] for i, k in enumerate(("x0", "x1", "y0", "y1", "pixels"))}
    runs["word"] = extend([np.asarray(r[3], np.int64) for r in refs], n) + np.repeat(first_word, n_runs)
    word_t = extend([np.asarray(r[2], np.int64).reshape(-1, 8) for r in refs], n)
    words = {k: word_t[:, i] for i, k in enumerate(("line", "first_run", "n_runs", "x", "y", "w", "h", "pixels"))}
    words["line"] = np.repeat(np.arange(n, dtype=np.int64), n_words)
    words["first_run"] = words["first_run"] + np.repeat(first_run, n_words)
    return lines, runs, words


# ---- the line crops ---------------------------------------------------------------------------------------------------------------------
CROP_SETTINGS = (8, 16, 0.0)        # set_line_crop: height, max_width, pad -- at most 128 bytes a crop
CROP_PW, CROP_PH = 97, 61


@functools.lru_cache(maxsize=None)
def crop_cases():
    """(plane, [(boxes (x, y, w, h), slope)] * K): a noise plane and K lines of different boxes and slopes, some leaving the plane."""
    plane = np.random.default_rng(97).integers(0, 256, (CROP_PH, CROP_PW), dtype=np.uint8)
    plane[0, 0], plane[CROP_PH - 1, CROP_PW - 1] = 0, 255
    lines = [([(10, 10, 40, 12)], 0.0), ([(5, 30, 12, 20), (22, 33, 10, 18)], 0.2), ([(50, 5, 30, 10)], -0.2), ([(0, 0, CROP_PW, CROP_PH)], 3.0),
             ([(-10, -5, 30, 12)], 0.1), ([(80, 50, 30, 20)], -0.4), ([(20, 20, 3, 40)], 0.0), ([(0, 25, CROP_PW, 6)], 0.05), ([(40, 40, 1, 1)], 1.0)]
    return plane, lines


@functools.lru_cache(maxsize=None)
def crop_refs():
    """Per case: (the record's fields (width, height, ax, ay, ux, uy, vx, vy), the crop's bytes) by the numpy contract."""
    plane, lines = crop_cases()
    out = []
    for boxes, slope in lines:
        g = CROP.geometry(boxes, slope, *CROP_SETTINGS)
        out.append((g, CROP.sample_grey(plane, g).reshape(-1)))
    return out


def crop_args(n=N):
    """(boxes (m, 4), first, count, slopes) of n lines."""
    _, lines = crop_cases()
    count, first = starts([len(b) for b, _ in lines], n)
    return extend([np.asarray(b, np.int64).reshape(-1, 4) for b, _ in lines], n), first, count, extend([[s] for _, s in lines], n)


def crop_expected(n=N):
    """({field: array over n lines} of the crop records, the crops' bytes back to back)."""
    refs = crop_refs()
    assert all(len(b) % 4 == 0 for _, b in refs)                        # (height 8: no padding between the crops)
    rec_t = extend([np.asarray([g], np.int64) for g, _ in refs], n)
    recs = {k: rec_t[:, i] for i, k in enumerate(("width", "height", "ax", "ay", "ux", "uy", "vx", "vy"))}
    recs["pix_off"] = starts([len(b) for _, b in refs], n)[1]
    return recs, extend([b for _, b in refs], n)
