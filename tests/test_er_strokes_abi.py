"""CPU checks of the stroke-width descriptor (STR_ER_WANT_STROKES, str_er_er_strokes): header, struct layout, exports, binding, the
C++ mirror and example, and the numpy / scipy reference of the GPU tests pinned on the closed forms of include/str_er.h."""
import math
import os
import re
import subprocess

import numpy as np
from scipy import ndimage

from stroke_ref import EIGHT, FOUR, depth, erosions, ridge, ridge_bitrows, stroke_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
HOST = os.path.join(ROOT, "scene-text-recognition_amd", "host")
FUNCS = ("str_er_result_strokes", "str_er_er_strokes")
FIELDS = [("depth_max", 0), ("ridge_pixels", 4), ("depth_sum", 8), ("ridge_depth_sum", 16), ("ridge_depth_sum2", 24)]


def test_header_declares_strokes():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+STR_ER_WANT_STROKES\s+\(65536u\)", txt)
    assert re.search(r"#define\s+STR_ER_ABI_VERSION\s+2\b", txt)
    assert re.search(r"typedef\s+struct\s+str_er_stroke\s*\{\s*uint32_t\s+depth_max;\s*uint32_t\s+ridge_pixels;\s*uint64_t\s+depth_sum;\s*"
                     r"uint64_t\s+ridge_depth_sum;\s*uint64_t\s+ridge_depth_sum2;\s*\}\s*str_er_stroke;", txt)
    assert re.search(r"const\s+str_er_stroke\s*\*\s*str_er_result_strokes\s*\(\s*const\s+str_er_result\s*\*\s*r\s*,\s*int32_t\s*\*\s*n\s*\)", txt)
    assert re.search(r"int\s+str_er_er_strokes\s*\(\s*str_er_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*plane\s*,\s*int32_t\s+w\s*,\s*int32_t\s+h\s*,"
                     r"\s*int64_t\s+stride\s*,\s*const\s+str_er_cand\s*\*\s*regions\s*,\s*int32_t\s+n\s*,\s*str_er_stroke\s*\*\s*out\s*\)", txt)


def test_stroke_layout_c99(tmp_path):
    src = tmp_path / "t.c"
    checks = "".join(f"typedef char off_{n}[offsetof(str_er_stroke, {n}) == {o} ? 1 : -1];\n" for n, o in FIELDS)
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n'
                   "typedef char size_ok[sizeof(str_er_stroke) == 32 ? 1 : -1];\n" + checks +
                   "typedef char flag_ok[STR_ER_WANT_STROKES == 65536u ? 1 : -1];\n"
                   "typedef char flags_apart[(STR_ER_WANT_STROKES & (STR_ER_WANT_SHAPES | STR_ER_WANT_MASKS | STR_ER_WANT_TEXT_MAP |"
                   " STR_ER_WANT_LINE_MAP | STR_ER_WANT_LINE_CROPS | STR_ER_WANT_LINE_GLYPHS)) == 0 ? 1 : -1];\n"
                   "typedef int (*strokes_fn)(str_er_ctx *, const uint8_t *, int32_t, int32_t, int64_t, const str_er_cand *, int32_t, str_er_stroke *);\n"
                   "int main(void) { size_ok a; flag_ok e; flags_apart d; strokes_fn f = str_er_er_strokes;\n"
                   "  const str_er_stroke *(*g)(const str_er_result *, int32_t *) = str_er_result_strokes;\n"
                   "  (void)a; (void)e; (void)d; (void)f; (void)g; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_library_exports_the_symbols(S):
    L = S.load_library()
    for name in FUNCS:
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS:
        assert re.search(r"\bT\s+" + name + r"\b", out), name


def test_binding_stroke_dtype(S):
    assert S.WANT_STROKES == 65536
    d = S.STROKE_DTYPE
    assert d.itemsize == 32 and [(n, d.fields[n][1]) for n in d.names] == FIELDS
    assert d["depth_max"] == np.dtype("<u4") and d["ridge_pixels"] == np.dtype("<u4")
    assert all(d[n] == np.dtype("<u8") for n in ("depth_sum", "ridge_depth_sum", "ridge_depth_sum2"))
    import inspect
    for m in ("text_detect", "text_detect_list"):
        assert inspect.signature(getattr(S.ERFilter, m)).parameters["want_strokes"].default is False
    assert hasattr(S.ERFilter, "er_strokes")


def test_cpp_mirror_and_example_compile(S, tmp_path):
    txt = open(os.path.join(HOST, "er_filter_hip.hpp")).read()
    assert "er_strokes(const Image8 &plane, const ERs &ers)" in txt
    libdir = os.path.dirname(S.lib_path())
    exe = str(tmp_path / "example_er_strokes")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(HOST, "example_er_strokes.cpp"), "-I", HOST,
                    "-I", os.path.join(ROOT, "include"), "-L", libdir, "-lstr_er_hip", f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    assert "STR_ER_WANT_STROKES" in open(os.path.join(HOST, "example_er_strokes.cpp")).read()
    assert "STR_ER_WANT_STROKES" not in open(os.path.join(HOST, "example_er_masks.cpp")).read()


# ---- the reference on masks with answers worked out by hand ------------------------------------------------------------------------

def _checked(m):
    """stroke_ref, with the ridge cross-checked against the bit-row form and D against the erosions' sizes."""
    m = np.asarray(m, bool)
    assert (ridge(m) == ridge_bitrows(m)).all()
    r = stroke_ref(m)
    e = erosions(m)
    assert r["depth_max"] == len(e) - 1
    assert r["depth_sum"] == sum(int(x.sum()) for x in e[:-1])
    d = depth(m)
    assert (d[m] >= 1).all() and (d[m] <= r["depth_max"]).all() and (d[~m] == 0).all()
    return r


def test_ref_bars_both_orientations():
    L = 31
    for t in range(1, 10):
        m = np.ones((t, L), bool)
        r = _checked(m)
        assert r == _checked(m.T)
        half = math.ceil(t / 2)
        rg = ridge(m)
        assert set(depth(m)[rg].tolist()) == {half}
        ys, xs = np.nonzero(rg)
        if t % 2:
            short = (t - 1) // 2
            assert sorted(set(ys.tolist())) == [t // 2]
        else:
            short = t // 2 - 1
            assert sorted(set(ys.tolist())) == [t // 2 - 1, t // 2]
        assert xs.min() == short and xs.max() == L - 1 - short
        assert r["ridge_pixels"] == (1 if t % 2 else 2) * (L - 2 * short)
        assert r["depth_max"] == half
        assert r["ridge_depth_sum"] == half * r["ridge_pixels"] and r["ridge_depth_sum2"] == half * half * r["ridge_pixels"]
        mean = r["ridge_depth_sum"] / r["ridge_pixels"]
        assert (2 * mean - 1 if t % 2 else 2 * mean) == t                       # the width from the mean depth
        assert r["ridge_depth_sum2"] / r["ridge_pixels"] - mean * mean == 0     # one width: no spread


def test_ref_squares():
    for n in range(1, 14):
        r = _checked(np.ones((n, n), bool))
        assert r["depth_max"] == math.ceil(n / 2)
        assert r["depth_sum"] == sum((n - 2 * k) ** 2 for k in range(n) if n - 2 * k > 0)
        assert r["ridge_pixels"] == (1 if n % 2 else 4)
        assert r["ridge_depth_sum"] == r["ridge_pixels"] * r["depth_max"]


def test_ref_single_pixel():
    one = {"depth_max": 1, "ridge_pixels": 1, "depth_sum": 1, "ridge_depth_sum": 1, "ridge_depth_sum2": 1}
    assert _checked(np.ones((1, 1), bool)) == one
    m = np.zeros((5, 7), bool)              # a pixel in a larger box: the box does not matter
    m[2, 3] = True
    assert _checked(m) == one


def test_ref_ring():
    # a ring 2 pixels thick round a hole: the hole's border erodes like the outer one, so the 4-erosion keeps only the four inner
    # corners (their 4-neighbours are all in M); they have depth 2, everything else depth 1, and the ridge is M less the 7 depth-1
    # neighbours of each corner
    m = np.ones((10, 12), bool)
    m[2:-2, 2:-2] = False
    r = _checked(m)
    corners = np.zeros_like(m)
    corners[[1, 1, -2, -2], [1, -2, 1, -2]] = True
    assert (depth(m) == np.where(corners, 2, m.astype(int))).all()
    assert r == {"depth_max": 2, "ridge_pixels": 72 - 4 * 7, "depth_sum": 72 + 4, "ridge_depth_sum": 4 * 2 + 40, "ridge_depth_sum2": 4 * 4 + 40}
    # 3 thick: depth 2 on the middle loop and the four inner corners, which together are the whole ridge
    m = np.ones((13, 15), bool)
    m[3:-3, 3:-3] = False
    r = _checked(m)
    mid = np.zeros_like(m)
    mid[1:-1, 1:-1] = True
    mid[2:-2, 2:-2] = False
    mid[[2, 2, -3, -3], [2, -3, 2, -3]] = True
    assert r["depth_max"] == 2 and set(depth(m)[ridge(m)].tolist()) == {2}
    assert (ridge(m) == mid).all() and r["ridge_pixels"] == int(mid.sum()) == 44 + 4


def test_ref_diagonal_band():
    # |x - y| < t: a diagonal stroke; away from its ends the ridge sits on one depth
    n = 48
    yy, xx = np.mgrid[0:n, 0:n]
    for t in (1, 2, 3, 5, 8):
        m = np.abs(xx - yy) < t
        _checked(m)
        d, rg = depth(m), ridge(m)
        inner = rg & (xx > 2 * t) & (xx < n - 2 * t) & (yy > 2 * t) & (yy < n - 2 * t)
        assert inner.any() and len(set(d[inner].tolist())) == 1, t


def test_ref_alternates_four_and_eight():
    # E_1 is the 4-erosion of M and E_2 the 8-erosion of E_1
    plus = np.zeros((5, 5), bool)
    plus[2, :] = plus[:, 2] = True
    e = erosions(plus)
    assert e[1].sum() == 1 and e[1][2, 2] and len(e) == 3
    sq = np.ones((5, 5), bool)
    e = erosions(sq)
    assert (e[1] == ndimage.binary_erosion(sq, structure=FOUR, border_value=0)).all() and e[1].sum() == 9
    assert (e[2] == ndimage.binary_erosion(e[1], structure=EIGHT, border_value=0)).all() and e[2].sum() == 1


def test_ref_random_shapes_bit_rows():
    rng = np.random.default_rng(5)
    n = 0
    for _ in range(30):
        h, w = rng.integers(1, 40, size=2)
        m = ndimage.gaussian_filter(rng.random((h, w)), 2) > 0.5
        if m.any():
            _checked(m)
            n += 1
    assert n > 10
