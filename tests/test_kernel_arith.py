"""The integer / floating-point shortcuts the round-4 kernels take, restated in numpy and checked against the plain forms they replace.

These are host-side restatements of device arithmetic (er_kernels.hip: k_nms's overlap test, k_classify's reciprocal divisions, packed histogram and LBP
bits, k_resize's 24-bit products and row walk): the GPU parity tests prove the kernels' results, these pin WHY the shortcuts are exact, over their whole
input ranges, on a machine without a GPU.
"""
import math

import numpy as np
import pytest


# ---- k_nms: (double)as / (double)ap > coef decided from the sign of as - coef * ap unless that is within 1e-9 * ap of 0 ------------------------------

def _ratio_gt_shortcut(a, p, coef):
    x, y = np.float64(a), np.float64(p)
    d = x - np.float64(coef) * y
    if abs(d) > 1e-9 * y:
        return bool(d > 0.0)
    return bool(x / y > np.float64(coef))


@pytest.mark.parametrize("coef", [0.7, 0.2, 0.25, 0.5, 0.9, 0.3, 1.0 / 3.0, 0.6999999999999999, 0.7000000000000001])
def test_overlap_test_without_the_division(coef):
    rng = np.random.default_rng(int(coef * 1e6) & 0xFFFF)
    # box areas of a 1920 x 1080 plane and of a 3840 x 2160 one; the adversarial cases sit next to coef * ap
    for ap in np.concatenate([rng.integers(1, 1920 * 1080 + 1, 3000), rng.integers(1, 3840 * 2160 + 1, 1000), np.arange(1, 400)]):
        ap = int(ap)
        mid = int(math.floor(coef * ap))
        for a in {max(1, mid - 1), max(1, mid), mid + 1, mid + 2, int(rng.integers(1, ap + 1))}:
            if a > ap:
                continue
            want = bool(np.float64(a) / np.float64(ap) > np.float64(coef))
            assert _ratio_gt_shortcut(a, ap, coef) == want, (a, ap, coef)


def test_overlap_test_on_exact_quotients():
    # quotients that ARE the coefficient (2/10 against 0.2 ...): the shortcut must fall through to the division
    for num, den, coef in [(2, 10, 0.2), (1, 4, 0.25), (7, 10, 0.7), (9, 10, 0.9), (1, 2, 0.5), (3, 10, 0.3)]:
        for k in range(1, 2000, 7):
            a, p = num * k, den * k
            assert _ratio_gt_shortcut(a, p, coef) == bool(np.float64(a) / np.float64(p) > np.float64(coef))


# ---- k_classify: divisions by multiplication ----------------------------------------------------------------------------------------------------------

def test_reciprocal_division_by_the_tile_width():
    # ii / dw for ii < dw * dh <= 676, dw <= 26: (ii * ceil(65536 / dw)) >> 16
    for dw in range(1, 27):
        rcp = (65536 + dw - 1) // dw
        ii = np.arange(0, 26 * 26, dtype=np.uint32)
        assert rcp < (1 << 24) and int(ii.max()) * rcp < (1 << 32)          # v_mul_u32_u24's operands, and its 32-bit result
        np.testing.assert_array_equal((ii * np.uint32(rcp)) >> 16, ii // dw)


def test_division_by_24_of_the_lbp_index():
    idx = np.arange(0, 24 * 24, dtype=np.uint32)
    np.testing.assert_array_equal((idx * np.uint32(2731)) >> 16, idx // 24)


def test_lbp_bits_are_the_sign_of_sum_minus_8v():
    rng = np.random.default_rng(7)
    v = rng.integers(0, 256, (20000, 8)).astype(np.int64)
    v[:2000] = rng.integers(100, 104, (2000, 8))            # near-flat neighbourhoods: many 8 v == sum cases
    s = v.sum(axis=1)
    want = np.zeros(len(v), np.uint32)
    for k in range(8):
        want |= ((8 * v[:, k] > s).astype(np.uint32) << k)
    code = np.zeros(len(v), np.uint32)
    for k in range(7, -1, -1):                              # v_alignbit(code, diff, 31) = (code << 1) | (diff >> 31), v7 first
        diff = (s - 8 * v[:, k]).astype(np.int32).view(np.uint32)
        code = (code << np.uint32(1)) | (diff >> np.uint32(31))
    np.testing.assert_array_equal(code, want)


def test_histogram_counted_into_packed_bytes_never_carries():
    # a 24 x 24 LBP image has four 12 x 12 cells: at most 144 pixels fall into one bin -- a byte holds it, no carry into the neighbouring bin
    rng = np.random.default_rng(11)
    for trial in range(50):
        codes = rng.integers(0, 256, (24, 24)) if trial else np.zeros((24, 24), np.int64)       # (all pixels one code: the worst case)
        row = np.zeros(256, np.uint32)                       # the ER's packed row: 1024 bins, a byte each
        hist = np.zeros(1024, np.uint32)
        for i in range(24):
            for j in range(24):
                b = (512 if i >= 12 else 0) + (256 if j >= 12 else 0) + int(codes[i, j])
                hist[b] += 1
                row[b >> 2] += np.uint32(1 << (8 * (b & 3)))
        assert hist.max() <= 144
        np.testing.assert_array_equal(row.view(np.uint8), hist.astype(np.uint8))


# ---- cv::resize's fixed-point bilinear: every product fits 24 bits, nothing is negative ----------------------------------------------------------------

def test_resize_products_fit_24_bits():
    f = np.linspace(0.0, 1.0, 100001, dtype=np.float32)[:-1]
    a1 = np.rint(f * np.float32(2048.0)).astype(np.int64)
    a0 = np.rint((np.float32(1.0) - f) * np.float32(2048.0)).astype(np.int64)
    assert a0.min() >= 0 and a1.min() >= 0 and a0.max() <= 2048 and a1.max() <= 2048
    assert (a0 + a1).max() <= 2049                          # (the two roundings can add up to 2049, never more)
    h = 255 * (a0 + a1)                                     # horizontal sum of two taps
    assert h.max() < (1 << 24)
    assert 2048 < (1 << 24) and (h >> 4).max() < (1 << 24) and (2048 * (h >> 4)).max() < (1 << 32)


def _row_table(dy, scale_y, sh):
    fy = np.float32((dy + 0.5) * scale_y - 0.5)
    sy = int(math.floor(fy))
    return min(max(sy, 0), sh - 1), min(max(sy + 1, 0), sh - 1)


def test_resize_rows_are_adjacent_or_equal():
    # what k_resize's row cache (and the classify resize's row table: bit 31 = "y1 is the next row") relies on: y1 is y0 or y0 + 1, rows never go back
    rng = np.random.default_rng(3)
    sizes = [(1080, 764), (764, 540), (540, 382), (382, 270), (270, 191), (191, 135), (135, 95), (2160, 1527)]
    sizes += [(int(s), int(d)) for s, d in zip(rng.integers(2, 1500, 200), rng.integers(1, 1500, 200))]
    for sh, dh in sizes:
        scale_y = 1.0 / (dh / sh)
        prev = (-1, -1)
        for dy in range(dh):
            ya, yb = _row_table(dy, scale_y, sh)
            assert yb in (ya, ya + 1)
            assert ya >= prev[0] and yb >= prev[1]
            prev = (ya, yb)


# ---- k_nms: a chain's winner, all members at once ---------------------------------------------------------------------------------------------------------

def _winner_sequential(areas, T):
    """src/ER.cpp:464-497 as the old kernel path walks it: i over the chain, trail = chain[i], lead = chain[i + T]."""
    n = len(areas)
    if n < 1 + T:
        return None
    best, best_st, best_a = 0, 0.0, 0
    for i in range(n - T):
        a, bb = areas[i], areas[i + T]
        with np.errstate(divide="ignore"):
            st = np.float64(a) / np.float64(bb - a)         # 0 denominator -> +inf, as in the reference
        if i == 0 or st > best_st:
            best, best_st, best_a = i, st, a
        elif st == best_st and a < best_a:
            best, best_a = i, a
    return best


def _winner_parallel(areas, T):
    """The round-4 form: every member whose T-th ancestor is in the chain has a stability; max of its bit pattern, then the lowest member."""
    n = len(areas)
    cand = []
    for i in range(n - T):
        a, bb = areas[i], areas[i + T]
        with np.errstate(divide="ignore"):
            st = np.float64(a) / np.float64(bb - a)
        cand.append((int(np.float64(st).view(np.uint64)), i))
    if not cand:
        return None
    top = max(c[0] for c in cand)
    return min(i for bits, i in cand if bits == top)        # (levels rise along a chain: the lowest level is the smallest index)


@pytest.mark.parametrize("T", [0, 1, 2, 3, 5])
def test_chain_winner_in_parallel_is_the_sequential_one(T):
    rng = np.random.default_rng(100 + T)
    for trial in range(4000):
        n = int(rng.integers(1, 40))
        # box areas along a chain never shrink; plateaus (equal boxes -> 0 denominators, equal stabilities) are common
        steps = rng.choice([0, 0, 1, 2, 3, 10, 100, 5000], n)
        areas = (int(rng.integers(1, 50)) + np.cumsum(steps)).tolist()
        assert _winner_parallel(areas, T) == _winner_sequential(areas, T), (areas, T)


# ---- parse_cascade's integer table (api_models.cpp): (h < T) ? A : B for 8-bit counts, T = ceil(thr) for dir +1, floor(thr) + 1 with the outputs swapped
# ---- for dir -1, NaN -> 0 / 1e9, T clamped to [0, 300], packed as dim | T << 10 ------------------------------------------------------------------------

def _table_entry(thr, dirn, vp, vn):
    if dirn == 1:
        T, A, B = (0.0 if math.isnan(thr) else math.ceil(thr) if math.isfinite(thr) else thr), vp, vn
    else:
        T, A, B = (1e9 if math.isnan(thr) else math.floor(thr) + 1.0 if math.isfinite(thr) else thr), vn, vp
    return int(min(max(T, 0.0), 300.0)), A, B


def _listed_thresholds():
    from cascade_cases import threshold_tokens
    return [float(t) for t in threshold_tokens()]


@pytest.mark.parametrize("dirn", [1, -1])
def test_integer_table_decides_like_the_stump(dirn):
    """For every count a byte can hold and every listed threshold (k, k +- 0.5, the doubles next to k at both ends of 0 .. 144, values past the
    clamp, a negative one, -0.0, the infinities, NaN): the table's entry gives what `h * dir < thr * dir ? vp : vn` gives."""
    h = np.arange(256, dtype=np.float64)
    vp, vn = 1.25, -0.75
    thrs = _listed_thresholds()
    assert any(math.isnan(t) for t in thrs) and math.inf in thrs and -math.inf in thrs and any(t == 0 and math.copysign(1, t) < 0 for t in thrs)
    for thr in thrs + [t + 0.25 for t in range(0, 146)] + [float(t) for t in range(-2, 147)]:
        T, A, B = _table_entry(thr, dirn, vp, vn)
        assert 0 <= T <= 300
        with np.errstate(invalid="ignore"):
            want = np.where(h * dirn < thr * dirn, vp, vn)
        got = np.where(h < T, A, B)
        np.testing.assert_array_equal(got, want, err_msg=f"thr {thr!r} dir {dirn}")


def test_integer_table_word_round_trips():
    dim, T = np.meshgrid(np.arange(1024, dtype=np.uint32), np.arange(301, dtype=np.uint32))
    w = dim | (T << np.uint32(10))
    assert int(w.max()) < (1 << 19)                         # 10 bits of dim, 9 of T: the readlane'd int stays positive
    np.testing.assert_array_equal(w & np.uint32(1023), dim)
    np.testing.assert_array_equal(w >> np.uint32(10), T)


# ---- k_classify's box arithmetic over every box NMS admits (0.1 < w / h < 2) -------------------------------------------------------------------------------

def _aran_dims(w, h):
    """OCR::ARAN's tile size (src/OCR.cpp:394-430) as k_classify computes it: the longer side becomes 26, the other (int)(26 * sqrt(ratio))"""
    w, h = np.asarray(w, np.float64), np.asarray(h, np.float64)
    wide = w > h
    k = (26.0 * np.sqrt(np.where(wide, h / w, w / h))).astype(np.int64)
    return np.where(wide, 26, k), np.where(wide, k, 26)


def _resize_mode(sw, sh, dw, dh):
    """er_device.h resize_geom: 0 copy, 1 exact 2 x 2 area, 2 fixed-point bilinear"""
    sx, sy = 1.0 / (dw / sw), 1.0 / (dh / sh)
    eps = np.finfo(np.float64).eps
    fast = (np.abs(sx - np.rint(sx)) < eps) & (np.abs(sy - np.rint(sy)) < eps) & (np.rint(sx) == 2) & (np.rint(sy) == 2)
    return np.where((dw == sw) & (dh == sh), 0, np.where(fast, 1, 2))


def test_box_arithmetic_over_every_admitted_box():
    w, h = np.meshgrid(np.arange(1, 601), np.arange(1, 601))
    ok = (w / h > 0.1) & (w / h < 2.0)
    w, h = w[ok], h[ok]
    dw, dh = _aran_dims(w, h)
    assert dw.min() >= 8 and dh.min() >= 8 and dw.max() == 26 and dh.max() == 26          # never 0: the dw > 0 && dh > 0 test is k_lbp_boxes' business
    assert ((dw == 26) | (dh == 26)).all()
    mode = _resize_mode(w.astype(np.float64), h.astype(np.float64), dw.astype(np.float64), dh.astype(np.float64))
    # copy: the box IS its tile; exact 2 x: the box is twice its tile both ways, nothing else comes within DBL_EPSILON of scale 2
    np.testing.assert_array_equal(mode == 0, (w == dw) & (h == dh))
    np.testing.assert_array_equal(mode == 1, (w == 2 * dw) & (h == 2 * dh))
    assert set(zip(w[mode == 0].tolist(), h[mode == 0].tolist())) >= {(26, 26), (25, 26), (26, 25)} and (np.maximum(w, h)[mode == 0] == 26).all()
    assert (np.maximum(w, h)[mode == 1] == 52).all()
    from cascade_cases import WANTED_SIZES
    ww, wh = np.array([s[0] for s in WANTED_SIZES]), np.array([s[1] for s in WANTED_SIZES])
    assert ((ww / wh > 0.1) & (ww / wh < 2.0)).all()
    wdw, wdh = _aran_dims(ww, wh)
    got = _resize_mode(ww.astype(np.float64), wh.astype(np.float64), wdw.astype(np.float64), wdh.astype(np.float64)).tolist()
    assert got == [0, 0, 1, 1, 1] + [2] * 13          # what tests/test_classify_edges.py assumes of its rectangles
    # the separable resize's tables: a column entry is (sx, sx1) in 16 bits each, a row entry the byte offset y0 * stride with bit 31 free for
    # "y1 is the next row"; 26 entries of each fit the wave's two halves
    assert dw.max() <= 32 and dh.max() <= 32 and int(w.max()) - 1 < (1 << 16)
    for stride, rows in ((3840, 2160), (7680, 4320)):
        tallest = int(math.ceil(0.8 * rows)) - 1            # NMS: h < 0.8 * rows
        assert max(int(h.max()) - 1, tallest - 1) * stride + stride < (1 << 31)


# ---- k_ocr_features (ocr_kernels.hip): the row index, the packed bit rows and the blur through a table of 7-bit patterns ---------------------------------

def test_ocr_row_index_from_a_float_reciprocal():
    # dy = (int)(((float)i + 0.5f) * (1.0f / dw)) for a pixel index i < dw * dh <= 900 of the ARAN(30) tile
    i = np.arange(900, dtype=np.float32)
    for dw in range(1, 31):
        inv = np.float32(1.0) / np.float32(dw)
        got = ((i + np.float32(0.5)) * inv).astype(np.int64)
        assert got.dtype == np.int64 and ((i + np.float32(0.5)) * inv).dtype == np.float32
        np.testing.assert_array_equal(got, np.arange(900) // dw, err_msg=f"dw {dw}")


def test_ocr_bit_of_four_bytes_gathered_by_a_multiplication():
    # ((((row >> c) & 0x01010101) * 0x00204081 >> 21) & 0xF): bit c of the four bytes of a word, in byte order, whatever the other bits hold
    rng = np.random.default_rng(21)
    for c in range(8):
        for pat in range(16):
            for other in [0, 0xFFFFFFFF] + rng.integers(0, 1 << 32, 20).tolist():
                row = int(other) & ~(0x01010101 << c) & 0xFFFFFFFF
                for b in range(4):
                    row |= ((pat >> b) & 1) << (8 * b + c)
                got = ((((row >> c) & 0x01010101) * 0x00204081 & 0xFFFFFFFF) >> 21) & 0xF           # (a 32-bit product: the high bits fall away)
                assert got == pat, (c, pat, hex(row))


def _reflect101(i, n):
    """oracle/er_oracle.c reflect101 (BORDER_REFLECT_101)"""
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
    return i


def _padded_row(bits):
    """The 36-bit row of L.rows: marks at bits 3 .. 32, reflected columns at 0 .. 2 and 33 .. 35"""
    bits &= 0x3FFFFFFF
    p = bits << 3
    p |= ((bits >> 3) & 1) | ((bits >> 2) & 1) << 1 | ((bits >> 1) & 1) << 2
    p |= ((bits >> 28) & 1) << 33 | ((bits >> 27) & 1) << 34 | ((bits >> 26) & 1) << 35
    return p


def test_ocr_bit_row_padding_is_reflect_101():
    rng = np.random.default_rng(22)
    for bits in [0, 0x3FFFFFFF, 1, 1 << 29, 0b1110, 0b0111 << 26] + rng.integers(0, 1 << 30, 300).tolist():
        p = _padded_row(int(bits))
        assert p < (1 << 36)
        for x in range(-3, 33):
            assert (p >> (x + 3)) & 1 == (int(bits) >> _reflect101(x, 30)) & 1, (hex(int(bits)), x)


_KG = (8, 28, 56, 72, 56, 28, 8)


def _g7():
    t = np.arange(128)
    return 255 * sum(_KG[k] * ((t >> k) & 1) for k in range(7))


def test_ocr_blur_table_fits_16_bits():
    g = _g7()
    assert g.max() == 255 * 256 < (1 << 16) and g[0] == 0 and g[0b0001000] == 255 * 72
    # the vertical pass of seven such entries: below 2^32, and 255 after the rounding shift at the most -- the clamp never acts
    s = 256 * int(g.max())
    assert s < (1 << 32) and (s + (1 << 15)) >> 16 == 255


def _blur_two_pass(m):
    """The oracle's blur (ero_chain_features_slope): a row pass in 8.8 fixed point, a column pass rounded to nearest from 16 fractional bits"""
    L = 30
    hrow = np.zeros((L, L), np.int64)
    for y in range(L):
        for x in range(L):
            hrow[y, x] = sum(int(m[y, _reflect101(x + k, L)]) * _KG[k + 3] for k in range(-3, 4))
    out = np.zeros((L, L), np.int64)
    for y in range(L):
        for x in range(L):
            s = sum(int(hrow[_reflect101(y + k, L), x]) * _KG[k + 3] for k in range(-3, 4))
            out[y, x] = min((s + (1 << 15)) >> 16, 255)
    return out


def _blur_kernel_form(m):
    """k_ocr_features: packed rows, s_g7 by 7-bit window, 8 (h0 + h6) + 28 (h1 + h5) + 56 (h2 + h4) + 72 h3"""
    L = 30
    g = _g7()
    rows = [_padded_row(sum(1 << x for x in range(L) if m[y, x])) for y in range(L)]
    out = np.zeros((L, L), np.int64)
    top = 0
    for x in range(L):
        h = [int(g[(rows[_reflect101(y, L)] >> x) & 127]) for y in range(-3, L + 3)]
        for y in range(L):
            h0, h1, h2, h3, h4, h5, h6 = h[y:y + 7]
            s = 8 * (h0 + h6) + 28 * (h1 + h5) + 56 * (h2 + h4) + 72 * h3
            top = max(top, (s + (1 << 15)) >> 16)
            out[y, x] = min((s + (1 << 15)) >> 16, 255)
    return out, top


def test_ocr_blur_by_table_is_the_two_pass_blur():
    rng = np.random.default_rng(23)
    maps = [np.zeros((30, 30), np.uint8), np.full((30, 30), 255, np.uint8)]
    for density in (0.03, 0.2, 0.5, 0.9):
        maps += [np.where(rng.random((30, 30)) < density, 255, 0).astype(np.uint8) for _ in range(3)]
    edge = np.zeros((30, 30), np.uint8)
    edge[0, :] = edge[29, :] = edge[:, 0] = edge[:, 29] = 255
    maps.append(edge)
    for m in maps:
        got, top = _blur_kernel_form(m)
        np.testing.assert_array_equal(got, _blur_two_pass(m))
        assert top <= 255
    assert _blur_kernel_form(maps[1])[0].max() == 255 and _blur_kernel_form(maps[1])[0].min() == 255
