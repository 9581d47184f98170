"""Planes made up for the sibling-tie passes behind the first k_nms pass, and a numpy census of k_nms's watch rule.

Every builder returns a uint8 plane for the parameters PRM below (thresh step 8, MIN_AREA 6, OVERLAP_COEF 0.3; the relevance planes: 0.7).  numpy
only: no GPU, no library.  (scene-text-recognition_amd/synth.py, which draws the double-L glyph of S-ties, is numpy alone and is loaded by path.)

  family        what it is                                                               what happens to it behind the first pass
  kept          the double-L glyph on grey 200                                           one relevant two-way tie; the pools of the two key rules differ and
                                                                                         the reference's order is the first pass's (largest key): walked, pool kept
  changed       the transpose of a kept plane                                            the reference's order is smallest key: walked, another pool of the same size
  settled       the glyph with three single pixels between the two L's                   one two-way tie, equal pools under every rule: k_alt_list lists it, the
                                                                                         opposite-rule pass clears it, it is not walked
  free / rect   grey 200 / one plain rectangle                                           no tie: 0 / 1 candidate
  noise         uniform noise 64 x 48                                                    many ties; the walk changes the SIZE of the pool
  grid          n double-L glyphs in cells, one of them with a third stroke if asked     2 n (+ 1) watched children: the watch list (NMS_WATCH_CAP) from both sides
  relevance     a box P with three thin strokes that each cover > 0.7 of it              one three-way tie at P (no opposite-rule pass), area(P) x coef on either
                                                                                         side of 0.64 rows x cols
"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("tie_planes_synth", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "scene-text-recognition_amd", "synth.py"))
synth = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(synth)

PRM = dict(step=8, min_area=6, max_area=900000, stability_t=2, overlap_coef=0.3)
REL_PRM = dict(PRM, overlap_coef=0.7)
BG = 200


# =================================================================================================================================
# the census: the watch rule of k_nms (er_nms.inl, "planes with ties") on a node table
# =================================================================================================================================
def watch_census(nodes, root, rows, cols, coef):
    """(number of watched children, parents that have them).  A non-root node i is watched iff box(i) / box(parent) > coef, its parent has at least two
    such children and box(parent) x coef < 0.8 cols x 0.8 rows x (1 + 1e-9).  `nodes`: a structured array with w, h, parent."""
    n = len(nodes)
    area = nodes["w"].astype(np.int64) * nodes["h"].astype(np.int64)
    par = nodes["parent"].astype(np.int64)
    idx = np.arange(n)
    nonroot = idx != root
    par = np.where(nonroot, par, idx)
    big = nonroot & (area.astype(np.float64) / area[par].astype(np.float64) > coef)
    per_parent = np.bincount(par[big], minlength=n)
    rel = area.astype(np.float64) * coef < 0.8 * cols * 0.8 * rows * (1.0 + 1e-9)
    watched = big & (per_parent[par] > 1) & rel[par]
    return int(watched.sum()), sorted(set(par[watched].tolist()))


def tie_parents(nodes, root, coef):
    """Parents with at least two children whose own box covers more than coef of theirs: where a tie CAN occur (see watch_census)."""
    n = len(nodes)
    area = nodes["w"].astype(np.int64) * nodes["h"].astype(np.int64)
    idx = np.arange(n)
    par = np.where(idx != root, nodes["parent"].astype(np.int64), idx)
    big = (idx != root) & (area.astype(np.float64) / area[par].astype(np.float64) > coef)
    per_parent = np.bincount(par[big], minlength=n)
    return {int(p): int(per_parent[p]) for p in np.flatnonzero(per_parent > 1)}


# =================================================================================================================================
# the builders
# =================================================================================================================================
def free_plane(rows, cols, grey=BG):
    return np.full((rows, cols), grey, np.uint8)


def rect_plane(rows, cols, x, y, w, h, grey=40):
    """One plain rectangle: a chain of three (rectangle, plane) is too short for T = 2 -- so a rim one level above it makes it a candidate."""
    p = free_plane(rows, cols)
    p[y:y + h, x:x + w] = grey + 16
    p[y + 1:y + h - 1, x + 1:x + w - 1] = grey + 8
    p[y + 2:y + h - 2, x + 2:x + w - 2] = grey
    return p


def glyph_plane(rows, cols, gw, gh, x0=4, y0=4):
    """The double-L glyph (strokes 3, fill 30) in a plane of grey 200: channel 1 of synth.draw_tie_glyph's picture."""
    img = np.full((rows, cols, 3), BG, np.uint8)
    synth.draw_tie_glyph(img, x0, y0, gw, gh, 3, 3, 30)
    return np.ascontiguousarray(img[:, :, 1])


def flipped(p, how):
    """how: 'lr', 'ud' (the pool is kept, like the plane's own), 'T', 'r180' (the walk changes the pool)."""
    return np.ascontiguousarray({"lr": p[:, ::-1], "ud": p[::-1, :], "T": p.T, "r180": p[::-1, ::-1]}[how])


KEPT_SIZES = ((48, 48, 28, 28), (64, 64, 40, 40), (51, 47, 30, 26), (52, 48, 30, 30), (40, 40, 24, 24), (32, 32, 20, 20))     # cols, rows, gw, gh


def kept_plane(cols=48, rows=48, gw=28, gh=28):
    return glyph_plane(rows, cols, gw, gh)


def changed_plane(cols=48, rows=48, gw=28, gh=28):
    """cols x rows: the transpose of the kept plane of rows x cols with a gh x gw glyph."""
    return flipped(glyph_plane(cols, rows, gh, gw), "T")


def settled_plane(rows=48, cols=48, g=28, x0=6, y0=6, transposed=False):
    """The glyph and three single pixels inside the box, between the two L's."""
    p = glyph_plane(rows, cols, g, g, x0, y0)
    s = g / 28.0
    for dy, grey in ((12, 112), (14, 104), (16, 128)):
        p[y0 + int(round(dy * s)), x0 + int(round(14 * s))] = grey
    return flipped(p, "T") if transposed else p


def noise_plane(seed, rows=48, cols=64):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)


def _staircase(p, x0, y0, x1, y1, grey):
    """A 4-connected one-pixel line from (x0, y0) to (x1, y1), x1 >= x0, y1 >= y0."""
    x, y = x0, y0
    p[y, x] = grey
    while (x, y) != (x1, y1):
        if (x - x0) * (y1 - y0) <= (y - y0) * (x1 - x0) and x < x1 or y == y1:
            x += 1
        else:
            y += 1
        p[y, x] = grey


def grid_plane(n, g=20, cell=28, per_row=16, triples=0, pad=(0, 0)):
    """n double-L glyphs of g x g, one per cell x cell cell, per_row a row; the first `triples` of them with a staircase between the L's: a third child
    whose box covers more than 0.3 of the glyph's.  pad = (rows, columns) of grey 200 added at the bottom / right."""
    n_rows = (n + per_row - 1) // per_row
    p = free_plane(n_rows * cell + pad[0], per_row * cell + pad[1])
    o = (cell - g) // 2
    plain = glyph_plane(cell, cell, g, g, o, o)
    triple = plain.copy()
    _staircase(triple, o + 5, o + 5, o + g - 6, o + g - 6, 40)
    for k in range(n):
        t = triple if k < triples else plain
        x0, y0 = (k % per_row) * cell, (k // per_row) * cell
        p[y0:y0 + cell, x0:x0 + cell] = t.T if k % 2 else t        # every second one transposed: neither key rule gives the reference's pool
    return p


def relevance_plane(rows, cols, pw, ph, lw, lh, third=True):
    """A box P of pw x ph (grey 80) at the plane's left / top edge inside Q (grey 150, two columns and -- where there is room -- two rows more), on
    grey 200.  In P two one-pixel L's (grey 30; left + bottom, top + right) with boxes of lw x lh each and, if `third`, a staircase between them."""
    assert lw <= pw - 4 and lh <= ph - 4 and pw + 2 <= cols and ph <= rows
    p = free_plane(rows, cols)
    p[0:min(rows, ph + 2), 0:pw + 2] = 150
    p[0:ph, 0:pw] = 80
    p[ph - 1 - lh:ph - 1, 1] = 30
    p[ph - 2, 1:1 + lw] = 30
    p[1, pw - 1 - lw:pw - 1] = 30
    p[1:1 + lh, pw - 2] = 30
    if third:
        _staircase(p, 3, 3, pw - 4, ph - 4, 30)
    return p
