"""k_pyr_level (er_pyr_level.inl) without a GPU: its arithmetic against cv::resize's formula, exhaustively, and a restatement of its dispatch rule and of
its row and chunk schedule, which keeps the shape list of tests/test_pyr_level.py honest (as resize_tile_forms does for k_resize in
tests/test_plane_builders.py).

The arithmetic the kernel relies on, each stated here on every value it can meet:
  * (left tap | right tap << 16) dot (a0 | a1 << 16) is cv::resize's int32 horizontal sum h; the kernel keeps hs = h & ~15 = (h >> 4) << 4;
  * the high 32 bits of the 24-bit product hs * (b << 12) are (b * (h >> 4)) >> 16, the vertical pass's product;
  * a0 + a1 = b0 + b1 = 2048 for every float32 fraction a shape produces, and then a pixel is at most 255 without the clamp, and two columns' sums share a
    register without a carry from the lower into the upper."""
import math

import numpy as np

PL_CH, PL_NR, PL_WORDS, PL_MAX_ROWS, PL_ROWS = 4, 7, 100, 32, 8        # er_pyr_level.inl
ROWS = (8, 16, 32)                                                              # the tile heights launch_pyr_level takes
SQRT2 = math.sqrt(2.0)


# ======================================================================================================================================
# the shapes of tests/test_pyr_level.py
# ======================================================================================================================================
def pyr_dims(w0, h0, level):
    """The size of a pyramid level (oracle/er_oracle.c, ero_pyr_dims)."""
    k = 2.0 ** (-0.5 * level)
    return max(int(math.floor(w0 * k + 0.5)), 1), max(int(math.floor(h0 * k + 0.5)), 1)


def _up4(n):
    return (n + 3) // 4 * 4


WIDTHS = [(_up4(round(dw * SQRT2)), dw) for dw in (255, 256, 257, 258, 259, 513)]          # (sw, dw): one partial x-tile, one full, a second, a third; every dw % 4


def heights(rows):
    """(sh, dh) for tile height `rows`: 1 (no reduction within (1, 1.5] exists: k_resize's), rows - 1, rows, rows + 1, 2 rows + 3 -- and 45 rows, which is
    three chunks and a row for the smallest tile and more for the others."""
    return [(max(round(dh * SQRT2), dh + 1), dh) for dh in (1, rows - 1, rows, rows + 1, 2 * rows + 3, 45)]


# (sh, sw, sstride), (dh, dw, dstride): the two smallest steps of a 1920 x 1080 pyramid and the first step of a 1030-wide plane, rows padded to 64 bytes as
# the plane pool has them
PYRAMID_STEPS = [((191, 339, 384), (135, 240, 256)), ((135, 240, 256), (95, 170, 192)), ((12, 1030, 1088), (8, 728, 768))]

# (sh, sw, sstride), (dh, dw): shapes launch_pyr_level must hand to k_resize
FALLBACK_SHAPES = [((20, 396, 396), (20, 263)),         # scale_x just above 1.5 (and no reduction in y)
                   ((30, 400, 400), (21, 266)),         # scale_x just above 1.5 alone
                   ((40, 100, 100), (60, 300)),         # upscale
                   ((16, 1032, 1032), (8, 516)),        # exact 2 x 2
                   ((12, 600, 600), (12, 600)),         # copy
                   ((30, 102, 102), (21, 72))]          # a source stride that is no multiple of 4


def all_kernel_shapes():
    """Every (sh, sw, sstride, dh, dw, dstride, rows) of the GPU test that is meant to reach k_pyr_level or to show that it is not reached.  The destination's
    stride is its width rounded up to a multiple of 4 (the plane pool pads rows to 64 bytes)."""
    out = []
    for rows in ROWS:
        for sh, dh in heights(rows):
            for sw, dw in WIDTHS:
                out.append((sh, sw, sw, dh, dw, _up4(dw), rows))
    for (sh, sw, ss), (dh, dw, ds) in PYRAMID_STEPS:
        out += [(sh, sw, ss, dh, dw, ds, rows) for rows in (0,) + ROWS]
    for (sh, sw, ss), (dh, dw) in FALLBACK_SHAPES:
        out.append((sh, sw, ss, dh, dw, _up4(dw), 0))
    return out


# ======================================================================================================================================
# cv::resize's tables (OpenCV's resize.cpp, 8UC1 INTER_LINEAR: float32 coefficient tables in 2048 fixed point)
# ======================================================================================================================================
def cv_tables(n_dst, n_src, clamp_fraction):
    """Taps and coefficients of one direction: (i, c0, c1) with i unclamped unless clamp_fraction (the x direction zeroes the fraction where it clamps)."""
    scale = 1.0 / (n_dst / n_src)
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    i = np.floor(f).astype(np.int64)
    f = f - i.astype(np.float32)
    if clamp_fraction:
        f = np.where((i < 0) | (i >= n_src - 1), np.float32(0.0), f).astype(np.float32)
        i = np.clip(i, 0, n_src - 1)
    one, k = np.float32(1.0), np.float32(2048.0)
    return i, np.rint((one - f) * k).astype(np.int64), np.rint(f * k).astype(np.int64), scale


def cv_pixel(r0, r1, b0, b1):
    """The vertical pass of cv::resize on two int32 horizontal sums (before its clamp to 255)."""
    return (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2


# ======================================================================================================================================
# the dispatch rule and the schedule of k_pyr_level, restated
# ======================================================================================================================================
def qualifies(sh, sw, sstride, dh, dw, dstride=None):
    """launch_pyr_level / pyr_level_fits: True when k_pyr_level takes the shape (plane addresses and pitches are dword-aligned in every buffer of the library)."""
    dstride = dw if dstride is None else dstride
    if (sh, sw) == (dh, dw) or sstride % 4 or dstride % 4 or sstride < 4 or sh > 0xFFFF or sh * sstride >= 1 << 32 or dh * dstride >= 1 << 32:
        return False
    x, _, _, scale_x = cv_tables(dw, sw, True)
    y, _, _, scale_y = cv_tables(dh, sh, False)
    if not (1.0 < scale_x <= 1.5 and 1.0 < scale_y <= 1.5):
        return False
    for dx in range(0, dw, 4):
        if x[min(dx + 3, dw - 1)] - x[dx] > 6:
            return False
    for tx0 in range(0, dw, 256):
        x_lo, x_hi = x[tx0] & ~3, min(x[min(tx0 + 255, dw - 1)] + 1, sw - 1)
        if (x_hi - x_lo) // 4 + 1 > PL_WORDS - 2:
            return False
    yc = np.clip(y, 0, sh - 1), np.clip(y + 1, 0, sh - 1)
    for dy in range(0, dh, PL_CH):
        if yc[1][min(dy + PL_CH - 1, dh - 1)] - yc[0][dy] + 1 > PL_NR:
            return False
    return True


def schedule(sh, sw, dh, dw, rows):
    """The kernel's walk down every tile row: [(first output row of the chunk, first staged source row, [(dy, ya, yb, sums computed)])].  A chunk is PL_CH
    output rows; its window is the PL_NR source rows from the upper tap of its first row on (clamped to the plane's last row when staged, which the taps
    are too).  The two rows of sums change roles with every output row (hA is the upper row on even rows of a tile, hB on odd ones) and are kept from chunk
    to chunk and not from tile to tile."""
    y, _, _, _ = cv_tables(dh, sh, False)
    ya, yb = np.clip(y, 0, sh - 1), np.clip(y + 1, 0, sh - 1)
    out = []
    for dy0 in range(0, dh, rows):
        held = [-1, -1]                                 # source rows whose sums hA / hB hold
        for c0 in range(dy0, min(dy0 + rows, dh), PL_CH):
            body = []
            for dy in range(c0, min(c0 + PL_CH, dy0 + rows, dh)):
                up = (dy - dy0) & 1
                computed = 0
                for slot, want in ((up, int(ya[dy])), (up ^ 1, int(yb[dy]))):
                    if held[slot] != want:
                        held[slot] = want
                        computed += 1
                body.append((dy, int(ya[dy]), int(yb[dy]), computed))
            out.append((c0, int(ya[c0]), body))
    return out


# ======================================================================================================================================
# tests
# ======================================================================================================================================
def test_dot_product_form_is_the_horizontal_sum():
    """All 2049 coefficient pairs, all (L, R) in [0, 255]^2: the packed dot product is cv::resize's int32 sum, and the kept form carries exactly its h >> 4."""
    L, R = (v.astype(np.int64) for v in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    pair = (L | R << 16).astype(np.uint32)
    for a1 in range(2049):
        a0 = 2048 - a1
        aa = np.uint32(a0 | a1 << 16)
        dot = ((pair & np.uint32(0xFFFF)).astype(np.uint64) * np.uint64(aa & np.uint32(0xFFFF)) + (pair >> np.uint32(16)).astype(np.uint64) * np.uint64(aa >> np.uint32(16)))
        assert int(dot.max()) < 1 << 24                                     # the kept form is a 24-bit factor
        h = (L * a0 + R * a1).astype(np.int32)                              # cv::resize: int32
        assert (dot.astype(np.int64) == h).all(), a1
        hs = dot.astype(np.int64) & 0xFFFFF0
        assert (hs >> 4 == h >> 4).all() and (hs & 15 == 0).all(), a1


def test_high_product_form_is_the_vertical_product_and_no_pixel_exceeds_255():
    """Every h >> 4 a horizontal sum can have (0 .. 255 * 2048 >> 4) against every coefficient 0 .. 2048: the high word of (hs) * (b << 12) is
    (b * (h >> 4)) >> 16.  With b0 + b1 = 2048 the pixel is at most 255 (exactly 255 at the top), and the two-column sum stays below 2^16."""
    hq = np.arange((255 * 2048 >> 4) + 1, dtype=np.uint64)
    top = int(hq[-1])
    worst = 0
    for b in range(2049):
        bs = np.uint64(b << 12)
        assert int(bs) < 1 << 24
        assert ((((hq << np.uint64(4)) * bs) >> np.uint64(32)) == ((np.uint64(b) * hq) >> np.uint64(16))).all(), b
        s = ((b * top) >> 16) + (((2048 - b) * top) >> 16) + 2              # (monotone in both sums: the top of both is the largest)
        assert s < 1 << 10
        worst = max(worst, s >> 2)
    assert worst == 255


def test_coefficients_sum_to_2048_on_every_shape():
    """a0 + a1 = b0 + b1 = 2048 on the float32 fractions of every shape of the GPU test, of a 1080p and a 4k pyramid, and on a fine grid of fractions."""
    shapes = [(sh, sw, dh, dw) for sh, sw, _, dh, dw, _, _ in all_kernel_shapes()]
    for w0, h0 in ((1920, 1080), (3840, 2160)):
        for l in range(1, 12):
            (w, h), (nw, nh) = pyr_dims(w0, h0, l - 1), pyr_dims(w0, h0, l)
            shapes.append((h, w, nh, nw))
    for sh, sw, dh, dw in shapes:
        for n_dst, n_src, cl in ((dw, sw, True), (dh, sh, False)):
            _, c0, c1, _ = cv_tables(n_dst, n_src, cl)
            assert (c0 + c1 == 2048).all() and c0.min() >= 0 and c1.min() >= 0, (sh, sw, dh, dw)
    f = np.concatenate([np.arange(4097, dtype=np.float32) / np.float32(4096.0), np.random.default_rng(3).random(1 << 21, dtype=np.float32)])
    f = f[f < 1]
    assert (np.rint((np.float32(1.0) - f) * np.float32(2048.0)) + np.rint(f * np.float32(2048.0)) == 2048).all()


def test_every_level_of_a_1080p_pyramid_qualifies():
    """The seven steps of the flagship batch's pyramid (rows padded to 64 bytes) are k_pyr_level's; the host's own tile height is one of the forced ones."""
    assert [pyr_dims(1920, 1080, l) for l in (5, 6, 7)] == [(339, 191), (240, 135), (170, 95)] and PL_ROWS in ROWS
    for l in range(1, 8):
        (sw, sh), (dw, dh) = pyr_dims(1920, 1080, l - 1), pyr_dims(1920, 1080, l)
        assert qualifies(sh, sw, (sw + 63) // 64 * 64, dh, dw, (dw + 63) // 64 * 64), l


def test_shape_list_reaches_the_kernel_and_its_edges(capsys):
    """Coverage guard: which shapes k_pyr_level takes, and that for every one of them every output row's two source rows lie in the staged window when the row
    is computed, every quad of columns within 7 bytes, every tile's window within the staged words.  The list reaches: every tile height; first and later
    x-tiles, full and partial; every dw % 4; partial last tiles and chunks; row pairs that straddle a chunk edge with one and with two new sums; a chunk edge
    inside a tile and at a tile's end; windows clamped at the last source row; the last tap clamped at sw - 1."""
    seen = dict(rows=set(), dw_mod=set(), partial_x=0, later_full_x=0, partial_chunk=0, straddle=set(), clamp_y=0, clamp_x=0, chunks_in_tile=0, fallback=0)
    for sh, sw, ss, dh, dw, ds, rows in all_kernel_shapes():
        if not qualifies(sh, sw, ss, dh, dw, ds):
            seen["fallback"] += 1
            continue
        x, a0, a1, _ = cv_tables(dw, sw, True)
        seen["clamp_x"] += int(x[-1] == sw - 1 or x[-1] + 1 == sw - 1)
        seen["dw_mod"].add(dw % 4)
        seen["partial_x"] += int(dw % 256 != 0)
        seen["later_full_x"] += int(dw >= 512)
        for r in ((rows,) if rows else (PL_ROWS,)):
            seen["rows"].add(r)
            sched = schedule(sh, sw, dh, dw, r)
            for i, (c0, win, body) in enumerate(sched):
                assert 0 <= win <= sh - 1
                seen["partial_chunk"] += int(len(body) < PL_CH)
                seen["chunks_in_tile"] = max(seen["chunks_in_tile"], (min(r, dh - c0 // r * r) + PL_CH - 1) // PL_CH)
                for k, (dy, ya, yb, computed) in enumerate(body):
                    assert win <= ya <= yb < win + PL_NR, (sh, sw, dh, dw, r, dy, win, ya, yb)
                    seen["clamp_y"] += int(yb == sh - 1 and ya == sh - 1 or win + PL_NR - 1 > sh - 1)
                    if k == 0 and c0 % r:
                        seen["straddle"].add(computed)
                    assert computed >= 1 or dy % r                                # (a tile's first row sums both its rows)
    with capsys.disabled():
        print("\nk_pyr_level shape list:", {k: (sorted(v) if isinstance(v, set) else v) for k, v in seen.items()})
    assert seen["rows"] == set(ROWS) and seen["dw_mod"] == {0, 1, 2, 3}
    assert seen["partial_x"] and seen["later_full_x"] and seen["partial_chunk"] and seen["clamp_y"] and seen["clamp_x"]
    assert seen["straddle"] >= {1, 2} and seen["chunks_in_tile"] >= 8
    assert seen["fallback"] >= len(FALLBACK_SHAPES) + len(WIDTHS) * len(ROWS)          # the dispatch edges and every dh = 1
    for (sh, sw, ss), (dh, dw) in FALLBACK_SHAPES:
        assert not qualifies(sh, sw, ss, dh, dw, _up4(dw)), (sh, sw, dh, dw)
    for (sh, sw, ss), (dh, dw, ds) in PYRAMID_STEPS:
        assert qualifies(sh, sw, ss, dh, dw, ds), (sh, sw, dh, dw)
