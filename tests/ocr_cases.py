"""Made-up boxes, planes and batches for tests/test_ocr_edges.py: the feature half of the OCR scorer (k_ocr_features, RotSrc /
make_rot_geom, k_ocr_list / k_ocr_list_from in ocr_kernels.hip) at its own edges.

Everything here is numpy and plain Python: the constants and the geometry are restated from the sources (ocr_kernels.hip,
str_er_api.cpp: make_rot_geom), the reference vectors come from the oracle (oracle/er_oracle.c), which the caller hands in.
Nothing here imports the product package.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import cascade_cases as cc

OCR_WAVES, OTSU_BLOCK, LIST_CHUNK, N_CU = 4, 64, 4096, 256          # ocr_device.h, k_ocr_otsu, k_ocr_list; an MI355X's compute units
OCR_BIG_PX = 4096                                                    # boxes above this many pixels take the queued histogram path
FEATURE_WGS_PER_CU = 3                                               # launch_ocr_features: one round of resident workgroups


# ---- reference vectors, one oracle call per distinct (plane, box, slope) -----------------------------------------------------------------
class Refs:
    def __init__(self, oracle):
        self.o, self.memo, self.planes = oracle, {}, {}

    def plane(self, name, make):
        if name not in self.planes:
            self.planes[name] = make()
        return self.planes[name]

    def q(self, name, plane, box, slope=0.0):
        key = (name, int(box[0]), int(box[1]), int(box[2]), int(box[3]), float(slope))
        if key not in self.memo:
            x, y, w, h = key[1:5]
            self.memo[key] = self.o.chain_features(plane[y:y + h, x:x + w], float(slope))
        return self.memo[key]

    def rows(self, name, plane, boxes, slopes=None):
        sl = np.zeros(len(boxes)) if slopes is None else np.broadcast_to(np.asarray(slopes, np.float64), (len(boxes),))
        return np.stack([self.q(name, plane, b, s) for b, s in zip(boxes, sl)])


# =================================================================================================================================
# 1. ARAN(30) target sizes
# =================================================================================================================================
ARAN_SIDE = 960
ARAN_LISTED_SMALLEST = [(1, 900), (1, 225), (1, 100), (4, 225), (1, 36), (1, 25), (49, 900), (16, 225), (9, 100), (1, 9), (121, 900), (4, 25),
                        (169, 900), (49, 225), (1, 4), (64, 225), (289, 900), (9, 25), (361, 900), (4, 9), (49, 100), (121, 225), (529, 900),
                        (16, 25), (25, 36), (169, 225), (81, 100), (196, 225), (841, 900), (1, 1)]
ARAN_TRUNCATED = [(169, 225), (338, 450), (507, 675), (676, 900), (169, 900)]
ARAN_ZERO_EDGE = [(1, 899), (1, 900), (1, 901), (1, 960)]


def aran_k(w, h, root=math.sqrt):
    """k of ARAN(30) as feat_aran computes it (root = math.sqrt) or as the reference writes it (root = lambda r: math.pow(r, 0.5))"""
    r1 = h / w if w > h else w / h
    return int(30.0 * root(r1))


@functools.lru_cache(None)
def aran_search(side=ARAN_SIDE):
    """(near, below, smallest): the pairs w <= h <= side with 30 sqrt(w / h) within 1e-9 of an integer, those among them whose
    truncation lands below that integer, and for every k = 1 .. 30 the pair with the smallest h (and w) that is near k."""
    h, w = np.meshgrid(np.arange(1, side + 1), np.arange(1, side + 1))
    keep = w <= h
    w, h = w[keep], h[keep]
    v = 30.0 * np.sqrt(w / h)
    k = np.rint(v)
    near = np.abs(v - k) < 1e-9
    w, h, v, k = w[near], h[near], v[near], k[near].astype(int)
    below = [(int(a), int(b)) for a, b, t, kk in zip(w, h, v, k) if int(t) < kk]
    smallest = {}
    for a, b, kk in zip(w, h, k):
        if kk not in smallest or (b, a) < (smallest[kk][1], smallest[kk][0]):
            smallest[int(kk)] = (int(a), int(b))
    return list(zip(w.tolist(), h.tolist())), below, [smallest[kk] for kk in range(1, 31)]


def aran_plane():
    """Random bytes, 960 x 960: the listed boxes reach a side of 960 (1 x 960, 1 x 901), the context's capacity is 1920 x 1080."""
    return np.random.default_rng(30).integers(0, 256, (ARAN_SIDE, ARAN_SIDE), dtype=np.uint8)


@functools.lru_cache(None)
def aran_boxes():
    """Every listed size upright and transposed, each at one of the plane's corners in turn."""
    sizes = []
    for (w, h) in ARAN_LISTED_SMALLEST + ARAN_TRUNCATED + ARAN_ZERO_EDGE:
        for s in ((w, h), (h, w)):
            if s not in sizes:
                sizes.append(s)
    out = []
    for i, (w, h) in enumerate(sizes):
        x, y = ((0, 0), (ARAN_SIDE - w, 0), (0, ARAN_SIDE - h), (ARAN_SIDE - w, ARAN_SIDE - h))[i % 4]
        out.append((x, y, w, h))
    return np.array(out, np.int32)


# =================================================================================================================================
# 2. resize forms and placement;  5. box counts
# =================================================================================================================================
FORM_W, FORM_H = 333, 201


def blob_plane(w, h, seed):
    """Blobs and strokes at several scales with a little noise on top: a binarised crop has borders in every direction."""
    rng = np.random.default_rng(seed)
    a = np.zeros((h, w))
    for cell, amp in ((16, 90.0), (5, 60.0), (2, 25.0)):
        g = rng.uniform(-1.0, 1.0, ((h + cell - 1) // cell + 1, (w + cell - 1) // cell + 1))
        a += amp * np.kron(g, np.ones((cell, cell)))[:h, :w]
    a += rng.uniform(-8.0, 8.0, (h, w))
    return np.clip(a + 128.0, 0, 255).astype(np.uint8)


def form_plane():
    return blob_plane(FORM_W, FORM_H, 31)


def resize_mode(sw, sh):
    """er_device.h resize_geom for ARAN(30)'s source sw x sh: 0 copy, 1 exact 2 x 2 area, 2 fixed-point bilinear"""
    k = aran_k(sw, sh)
    dw, dh = (30, k) if sw > sh else (k, 30)
    if dw <= 0 or dh <= 0:
        return -1
    if (dw, dh) == (sw, sh):
        return 0
    sx, sy = 1.0 / (dw / sw), 1.0 / (dh / sh)
    eps = np.finfo(np.float64).eps
    fast = abs(sx - round(sx)) < eps and abs(sy - round(sy)) < eps and round(sx) == 2 and round(sy) == 2
    return 1 if fast else 2


@functools.lru_cache(None)
def form_boxes():
    sizes = [(w, h) for w in (29, 30, 31, 59, 60, 61) for h in (29, 30, 31, 59, 60, 61)] + [(1, 1), (1, 2), (2, 1), (2, 2)]
    out = []
    for (w, h) in sizes:
        for x, y in ((0, 0), (FORM_W - w, 0), (0, FORM_H - h), (FORM_W - w, FORM_H - h)):
            out.append((x, y, w, h))
    out.append((0, 0, FORM_W, FORM_H))
    return np.array(out, np.int32)


COUNTS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)
N_MANY = 3100


@functools.lru_cache(None)
def count_boxes():
    """31 small distinct boxes of the form plane, repeated to 3100: every row has one of 31 reference vectors."""
    rng = np.random.default_rng(32)
    short = []
    while len(short) < 31:
        w, h = int(rng.integers(3, 25)), int(rng.integers(3, 25))
        b = (int(rng.integers(0, FORM_W - w + 1)), int(rng.integers(0, FORM_H - h + 1)), w, h)
        if b not in short:
            short.append(b)
    return np.array(short * (N_MANY // 31), np.int32)


# =================================================================================================================================
# 3. content forms
# =================================================================================================================================
def pack(rois, width=640, gap=2, fill=128):
    """The ROIs on one plane, shelf by shelf: (plane, boxes xywh in the order given)."""
    shelf = cc._Shelf(0, 0, width, 1 << 20, gap)
    at = []
    for r in rois:
        h, w = r.shape
        at.append(shelf.put(w, h) + (w, h))
    rows = max(y + h for (_, y, _, h) in at)
    plane = np.full((rows, width), fill, np.uint8)
    for r, (x, y, w, h) in zip(rois, at):
        plane[y:y + h, x:x + w] = r
    return plane, np.array(at, np.int32)


CONST_VALUES = (0, 1, 254, 255)
CONST_SIZES = ((30, 30), (7, 7), (60, 60), (40, 13), (30, 29), (60, 10), (13, 40), (29, 30), (10, 60))      # square, wide, tall
THREE_LEVEL_SIZES = ((21, 10), (64, 8), (65, 8), (65, 64), (257, 20))     # one wave with several rows a pass, 64 wide, wide, wide + queued, widest + queued
THREE_LEVELS = ((10, 100, 190), (0, 127, 254), (1, 128, 255), (50, 51, 52), (254, 127, 0))
RAMP_SHIFTS = tuple(range(12))


def three_level(w, h, levels):
    """Columns of levels[0] | levels[1] | levels[2], the outer two equally wide: the class variances of the two thresholds
    between them are mirror images, and the scan's strict `>` (or the last bit of its f64 sums) decides."""
    n = w // 3
    r = np.full((h, w), levels[1], np.uint8)
    r[:, :n], r[:, w - n:] = levels[0], levels[2]
    return r


def ramp(shift, w=256, h=16):
    """Grey level = (column + shift) mod 256: every level is populated by one column whatever the shift, so the threshold stays where it
    is (Otsu follows a shift of the levels, not a rotation of them) and one column enters the foreground while another leaves it."""
    return np.broadcast_to(((np.arange(w) + shift) % 256).astype(np.uint8), (h, w)).copy()


def raster_ramp(shift, side):
    """Grey levels 0 .. 255 in raster order over side x side pixels (a level holds side * side / 256 consecutive pixels), rotated like
    ramp(): in the copy (30) and exact-2x (60) forms a threshold one level off moves that many pixels of the tile."""
    lv = (np.arange(side * side) * 256) // (side * side)
    return ((lv + shift) % 256).astype(np.uint8).reshape(side, side)


RASTER_SHIFTS = tuple(range(12))


def shapes30():
    """Dark (0) foreground on 255, 30 x 30: the copy form hands them to the direction marks pixel for pixel."""
    def blank():
        return np.full((30, 30), 255, np.uint8)
    out = {}
    yy, xx = np.mgrid[0:30, 0:30]
    a = blank(); a[(yy + xx) % 2 == 0] = 0; out["checkerboard"] = a
    a = blank(); a[(yy + xx) % 2 == 1] = 0; out["checkerboard, other phase"] = a
    a = blank(); a[11, 17] = 0; out["single pixel"] = a
    a = blank(); a[0, 0] = 0; out["single pixel in the corner"] = a
    a = blank(); a[14, :] = 0; out["horizontal line"] = a
    a = blank(); a[0, :] = 0; out["horizontal line on the top border"] = a
    a = blank(); a[:, 9] = 0; out["vertical line"] = a
    a = blank(); a[:, 29] = 0; out["vertical line on the right border"] = a
    a = blank(); a[yy == xx] = 0; out["diagonal"] = a
    a = blank(); a[yy == 29 - xx] = 0; out["anti-diagonal"] = a
    a = blank(); a[4:26, 4:26] = 0; a[8:22, 8:22] = 255; out["ring"] = a
    a = blank(); a[:, :] = 0; a[1:29, 1:29] = 255; out["ring on the border"] = a
    a = np.zeros((30, 30), np.uint8); a[13, 13] = 255; out["full tile with a hole"] = a
    a = np.zeros((30, 30), np.uint8); a[0, 0] = 255; out["full tile with a hole in the corner"] = a
    return out


@functools.lru_cache(None)
def content_cases():
    """(names, plane, boxes)"""
    rng = np.random.default_rng(33)
    names, rois = [], []
    for v in CONST_VALUES:
        for (w, h) in CONST_SIZES:
            names.append(f"const {v} {w}x{h}"); rois.append(np.full((h, w), v, np.uint8))
    for (w, h) in ((30, 30), (60, 60), (41, 23), (23, 41), (64, 64)):
        for (lo, hi) in ((60, 200), (0, 255), (127, 128)):
            names.append(f"two-level {lo}/{hi} {w}x{h}")
            rois.append(np.where(np.kron(rng.random(((h + 2) // 3, (w + 2) // 3)) < 0.5, np.ones((3, 3), bool))[:h, :w], lo, hi).astype(np.uint8))
    for s in RAMP_SHIFTS:
        names.append(f"ramp {s}"); rois.append(ramp(s))
    for side in (30, 60):
        for sh in RASTER_SHIFTS:
            names.append(f"raster ramp {side} {sh}"); rois.append(raster_ramp(sh, side))
    for (w, h) in THREE_LEVEL_SIZES:
        for lv in THREE_LEVELS:
            names.append(f"three-level {lv} {w}x{h}"); rois.append(three_level(w, h, lv))
    for n, a in shapes30().items():
        names.append("shape " + n); rois.append(a)
        names.append("shape 2x " + n); rois.append(np.kron(a, np.ones((2, 2), np.uint8)))
    plane, boxes = pack(rois)
    return names, plane, boxes


# =================================================================================================================================
# 4. slant
# =================================================================================================================================
def c_round(x):
    """C's round(): half away from zero"""
    a = abs(x)
    r = math.floor(a)
    if a - r >= 0.5:
        r += 1
    return int(math.copysign(r, x))


def rot_geom(w, h, slope):
    """make_rot_geom (str_er_api.cpp), i.e. OCR::rotate_mat's canvas (src/OCR.cpp:256-290): dict(on, crop, ch, rw, rh, full_h)"""
    if not abs(slope) > 0.01:
        return dict(on=0, crop=0, ch=0, rw=w, rh=h, full_h=h)
    rad = math.atan2(slope, 1.0)
    x0, y0 = int((w - 1) / 2.0), int((h - 1) / 2.0)
    cx, cy = (0 - x0, (w - 1) - x0, (w - 1) - x0, 0 - x0), (0 - y0, 0 - y0, (h - 1) - y0, (h - 1) - y0)
    nx = [c_round(cx[k] * math.cos(rad) - cy[k] * math.sin(rad)) for k in range(4)]
    ny = [c_round(cx[k] * math.sin(rad) + cy[k] * math.cos(rad)) for k in range(4)]
    full_h = max(ny) - min(ny) + 1
    ch, crop = int((nx[1] - nx[0]) * math.tan(rad) * 0.5), 1
    if full_h - 2 * ch <= 0:
        ch, crop = 0, 0
    return dict(on=1, crop=crop, ch=ch, rw=max(nx) - min(nx) + 1, rh=full_h - 2 * ch, full_h=full_h)


def raw_crop_height(w, h, slope):
    """rotate_mat's crop_height before the fall-back is considered, and the uncropped canvas height"""
    rad = math.atan2(slope, 1.0)
    x0, y0 = int((w - 1) / 2.0), int((h - 1) / 2.0)
    cx, cy = (0 - x0, (w - 1) - x0, (w - 1) - x0, 0 - x0), (0 - y0, 0 - y0, (h - 1) - y0, (h - 1) - y0)
    nx = [c_round(cx[k] * math.cos(rad) - cy[k] * math.sin(rad)) for k in range(4)]
    ny = [c_round(cx[k] * math.sin(rad) + cy[k] * math.cos(rad)) for k in range(4)]
    return int((nx[1] - nx[0]) * math.tan(rad) * 0.5), max(ny) - min(ny) + 1


@functools.lru_cache(None)
def fallback_shapes(slope, side=160):
    """The shapes w, h <= side whose cropped canvas would have no rows (the uncropped fall-back of src/OCR.cpp:285-289), in (w, h) order"""
    out = []
    for w in range(1, side + 1):
        for h in range(1, side + 1):
            ch, full = raw_crop_height(w, h, slope)
            if full - 2 * ch <= 0:
                out.append((w, h))
    return out


SLANT_W, SLANT_H = 320, 240
NEAR = [0.0, 0.01, -0.01, float(np.nextafter(0.01, 1)), float(np.nextafter(0.01, 0)), float(np.nextafter(-0.01, -1)), float(np.nextafter(-0.01, 0))]
STEEP = [s * m for m in (0.8, 1.0, 1.5, 2.0, 5.0, 50.0) for s in (1, -1)]
STEEP_SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 7), (7, 1), (1, 160), (160, 1), (3, 5), (30, 30), (60, 60), (31, 17), (17, 31), (100, 20), (20, 100),
               (159, 37), (160, 160)]
MAX_CANVAS = 4_000_000


def slant_plane():
    return blob_plane(SLANT_W, SLANT_H, 34)


def _at(i, w, h):
    return ((0, 0), (SLANT_W - w, 0), (0, SLANT_H - h), (SLANT_W - w, SLANT_H - h), ((SLANT_W - w) // 2, (SLANT_H - h) // 2))[i % 5]


@functools.lru_cache(None)
def slant_cases():
    """{family: (boxes, slopes)}"""
    fam = {}
    sizes = [(50, 40), (30, 30), (61, 5), (5, 61), (1, 1)]
    fam["switch"] = [(w, h, s) for (w, h) in sizes for s in NEAR]
    fam["steep"] = [(w, h, s) for (w, h) in STEEP_SIZES for s in STEEP]
    fb = [(58, 1, 0.8), (122, 1, 0.8)]
    f15, f50 = fallback_shapes(1.5), fallback_shapes(5.0)
    fb += [(w, h, 1.5) for (w, h) in (f15[:3] + f15[-2:])]
    fb += [(w, h, 5.0) for (w, h) in (f50[:4] + f50[len(f50) // 2:len(f50) // 2 + 3] + f50[-3:])]
    fam["fallback"] = fb
    fam["negative ch"] = [(100, 20, -0.5), (100, 20, -5.0), (160, 9, -1.0), (37, 37, -0.3), (150, 150, -2.0), (64, 1, -0.8)]
    one = []
    for s in (0.8, -0.8, 1.0, 5.0, -5.0, 50.0, -50.0, 0.02, -0.02):
        for (w, h) in ((1, 1), (1, 2), (2, 1), (1, 3), (3, 1), (2, 2), (1, 9), (9, 1), (40, 1), (1, 40), (2, 3), (3, 2)):
            g = rot_geom(w, h, s)
            if g["rw"] == 1 or g["rh"] == 1:
                one.append((w, h, s))
    fam["one wide or high"] = one
    out = {}
    for name, lst in fam.items():
        boxes = np.array([_at(i, w, h) + (w, h) for i, (w, h, _) in enumerate(lst)], np.int32)
        out[name] = (boxes, np.array([s for (_, _, s) in lst], np.float64))
    return out


@functools.lru_cache(None)
def mixed_wave_case():
    """Groups of four consecutive boxes (one workgroup's four waves): four different slopes in each, rotated and unrotated ones side by side."""
    rng = np.random.default_rng(35)
    patterns = [(0.0, 0.3, -0.7, 0.005), (1.5, 0.01, -0.2, -0.004), (0.25, -0.01, 0.0, -5.0), (0.009, 0.8, 0.011, -0.8), (0.0, 2.0, 0.002, -0.05)]
    boxes, slopes = [], []
    for g in range(40):
        for s in patterns[g % len(patterns)]:
            w, h = int(rng.integers(2, 70)), int(rng.integers(2, 70))
            boxes.append((int(rng.integers(0, SLANT_W - w + 1)), int(rng.integers(0, SLANT_H - h + 1)), w, h))
            slopes.append(s)
    return np.array(boxes, np.int32), np.array(slopes, np.float64)


# =================================================================================================================================
# 6. batches for the lister
# =================================================================================================================================
# A plane of 200 with dark shapes of at most 2 x 2 pixels on a 3-pixel grid, values 40 .. 43 (one level at thresh_step 8): every shape is one
# region with its exact box, pooled at RECT_PRM, in raster order of the slots (a 2 x 1 box would not be: NMS wants w / h < 2).  What
# ERFilter::classify sees of a shape is bin 0 of its LBP histogram (code 0 of the first cell): 144 for a constant box, 12 .. 48 for the
# shapes called strong here, 53 .. 93 for the weak ones, 120 for the last pool-only one -- so a one-stump strong cascade `bin 0 < 52` and a
# one-stump weak cascade `bin 0 < 100` make the classes below.
LIST_W, LIST_H, PITCH = 256, 192, 3
SLOTS = (LIST_W // PITCH) * (LIST_H // PITCH)
KINDS = {"dot40": ([[40]], 0), "dot41": ([[41]], 0), "dot43": ([[43]], 0), "rows": ([[40, 40], [43, 43]], 0), "flat": ([[42, 42], [42, 42]], 0),
         "s_v": ([[43], [40]], 1), "s_q": ([[43, 40], [40, 43]], 1), "s_cols": ([[40, 43], [40, 43]], 1), "s_l": ([[40, 200], [40, 40]], 1),
         "w_v": ([[40], [43]], 2), "w_q": ([[40, 43], [43, 40]], 2), "w_v2": ([[41], [42]], 2), "w_grad": ([[40, 41], [42, 43]], 2), "w_l": ([[40, 40], [40, 200]], 2)}
DOTS = ("dot40", "dot41", "rows", "dot43", "flat")
LISTED = ("s_v", "w_v", "s_q", "w_q", "s_cols", "w_v2", "s_l", "w_grad", "w_l")
MIXED = ("dot40", "s_v", "w_v", "dot41", "rows", "s_q", "w_q", "dot43", "s_cols", "w_v2", "flat", "s_l", "w_grad", "w_l")
FIRST, LAST = "s_v", "w_q"


def list_cascades():
    strong = cc.Cascade(True, [1], ["0"], [(1.0, 0, "52", 1.0, -1.0)])
    weak = cc.Cascade(True, [1], ["0"], [(1.0, 0, "100", 1.0, -1.0)])
    return strong, weak


def shape_plane(kinds):
    """The plane with these shapes in its slots, in raster order; (plane, expected classes)"""
    assert len(kinds) <= SLOTS
    img = np.full((LIST_H, LIST_W), 200, np.uint8)
    per_row = LIST_W // PITCH
    for i, k in enumerate(kinds):
        a = np.array(KINDS[k][0], np.uint8)
        y, x = PITCH * (i // per_row), PITCH * (i % per_row)
        img[y:y + a.shape[0], x:x + a.shape[1]] = a
    return img, np.array([KINDS[k][1] for k in kinds], np.uint8)


def _cyc(seq, n, start=0):
    return [seq[(start + i) % len(seq)] for i in range(n)]


@functools.lru_cache(None)
def list_batches():
    """{name: [kinds of plane 0, kinds of plane 1, ...]}"""
    b = {}
    b["1"] = [[FIRST]]
    for n in (4095, 4096, 4097):
        b[str(n)] = [_cyc(MIXED, n, n)]
    b["8192"] = [_cyc(MIXED, 4096), _cyc(MIXED, 4096, 3)]
    b["8193"] = [_cyc(MIXED, 4096, 5), _cyc(MIXED, 4097, 1)]
    b["five chunks and more"] = [_cyc(MIXED, 4200, p) for p in range(5)]
    b["none listed"] = [_cyc(DOTS, 4097)]
    b["all listed"] = [_cyc(LISTED, 4097)]
    b["only the first"] = [[FIRST] + _cyc(DOTS, 4095), _cyc(DOTS, 4097)]
    b["only the last"] = [_cyc(DOTS, 4096), _cyc(DOTS, 4096) + [LAST]]
    b["empty middle chunk"] = [_cyc(MIXED, 4096), _cyc(DOTS, 4096, 1), _cyc(MIXED, 4096, 2)]
    return b


LIST_TOTALS = {"1": 1, "4095": 4095, "4096": 4096, "4097": 4097, "8192": 8192, "8193": 8193, "five chunks and more": 21000, "none listed": 4097,
               "all listed": 4097, "only the first": 8193, "only the last": 8193, "empty middle chunk": 12288}


@functools.lru_cache(None)
def list_planes(name):
    """(planes (n, H, W), expected classes in candidate order)"""
    made = [shape_plane(tuple(k)) for k in list_batches()[name]]
    return np.stack([m[0] for m in made]), np.concatenate([m[1] for m in made])


# ---- planes with NMS sibling ties (the candidates of a re-made plane are listed by k_ocr_list_from) ----
TIE_PRM = dict(step=8, min_area=6, max_area=900000, stability_t=2, overlap_coef=0.3)       # test_classify_edges.py's
TIE_W, TIE_H = 240, 160


@functools.lru_cache(None)
def tie_batch():
    rng = np.random.default_rng(36)
    return np.stack([rng.integers(0, 256, (TIE_H, TIE_W), dtype=np.uint8) for _ in range(2)])
