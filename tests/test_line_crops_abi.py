"""CPU checks of the line crops (STR_ER_WANT_LINE_CROPS / _GLYPHS, str_er_line_crops, str_er_line_crop_geometry): header, struct
layout, exports, binding, the host geometry against a numpy restatement of the contract, and the numpy sampler the GPU tests use.
The reference functions here (geometry, sample_grey, sample_glyph) are the contract of include/str_er.h written in numpy."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
HOST = os.path.join(ROOT, "scene-text-recognition_amd", "host")
FUNCS = ("str_er_result_line_crops", "str_er_result_line_crop_pixels", "str_er_result_line_glyph_pixels", "str_er_set_line_crop",
         "str_er_line_crop_geometry", "str_er_line_crops")


def _llround(x: float) -> int:
    """C llround: halves away from zero (exact: x - floor(x) is exact for doubles of this size)."""
    f = np.floor(x)
    d = x - f
    return int(f) + (1 if d > 0.5 or (d == 0.5 and x > 0) else 0)


def geometry(boxes, slope, height=32, max_width=1024, pad=0.125):
    """The str_er_line_crop of one line: (width, height, ax, ay, ux, uy, vx, vy), f64 in the order of the header."""
    s = float(slope) if np.isfinite(slope) else 0.0
    r = np.sqrt(1.0 + s * s)
    dx, dy, nx, ny = 1.0 / r, s / r, -s / r, 1.0 / r
    us, vs = [], []
    for (x, y, w, h) in np.asarray(boxes, np.int64).reshape(-1, 4):
        for cx in (float(x), float(x + w)):
            for cy in (float(y), float(y + h)):
                us.append(cx * dx + cy * dy)
                vs.append(cx * nx + cy * ny)
    u0, u1, v0, v1 = min(us), max(us), min(vs), max(vs)
    p = pad * (v1 - v0)
    U0, U1, V0, V1 = u0 - p, u1 + p, v0 - p, v1 + p
    kv = (V1 - V0) / height
    width = int(min(max_width, max(1.0, np.ceil((U1 - U0) / kv))))
    ku = (U1 - U0) / width
    ax = U0 * dx + V0 * nx + 0.5 * ku * dx + 0.5 * kv * nx - 0.5
    ay = U0 * dy + V0 * ny + 0.5 * ku * dy + 0.5 * kv * ny - 0.5
    fx = [_llround(65536.0 * v) for v in (ax, ay, ku * dx, ku * dy, kv * nx, kv * ny)]
    return (width, height, *fx)


def _coords(g):
    """Per output pixel (height, width): sx, sy in int64."""
    width, height, ax, ay, ux, uy, vx, vy = [int(v) for v in g]
    i = np.arange(width, dtype=np.int64)[None, :]
    j = np.arange(height, dtype=np.int64)[:, None]
    return ax + i * ux + j * vx, ay + i * uy + j * vy


def sample_grey(plane, g):
    """The grey crop of geometry g on one plane: integer bilinear, taps clamped into the plane."""
    P = np.asarray(plane).astype(np.int64)
    ph, pw = P.shape
    sx, sy = _coords(g)
    x0, y0 = sx >> 16, sy >> 16
    fx, fy = (sx >> 8) & 255, (sy >> 8) & 255
    xa, xb = np.clip(x0, 0, pw - 1), np.clip(x0 + 1, 0, pw - 1)
    ya, yb = np.clip(y0, 0, ph - 1), np.clip(y0 + 1, 0, ph - 1)
    top = P[ya, xa] * (256 - fx) + P[ya, xb] * fx
    bot = P[yb, xa] * (256 - fx) + P[yb, xb] * fx
    return ((top * (256 - fy) + bot * fy + 32768) >> 16).astype(np.uint8)


def sample_glyph(union, g):
    """The glyph crop of geometry g: 255 where the nearest source pixel lies in the plane and in `union` (bool, plane-sized)."""
    ph, pw = union.shape
    sx, sy = _coords(g)
    xn, yn = (sx + 32768) >> 16, (sy + 32768) >> 16
    inside = (xn >= 0) & (xn < pw) & (yn >= 0) & (yn < ph)
    hit = np.zeros(xn.shape, bool)
    hit[inside] = union[yn[inside], xn[inside]]
    return np.where(hit, 255, 0).astype(np.uint8)


def fields(rec):
    return tuple(int(rec[k]) for k in ("width", "height", "ax", "ay", "ux", "uy", "vx", "vy"))


# ---- header, layout, exports, binding ---------------------------------------------------------------------------------------------

def test_header_declares_line_crops():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+STR_ER_WANT_LINE_CROPS\s+2048u\b", txt)
    assert re.search(r"#define\s+STR_ER_WANT_LINE_GLYPHS\s+4096u\b", txt)
    assert re.search(r"#define\s+STR_ER_ABI_VERSION\s+2\b", txt)
    flags = [int(v) for v in re.findall(r"#define\s+STR_ER_(?:STAGE|WANT|GROUP)_\w+\s+(\d+)u", txt)]
    assert 2048 in flags and 4096 in flags
    others = 0
    for v in flags:
        if v not in (2048, 4096, 7):
            others |= v
    assert others & (2048 | 4096) == 0 and others <= 2047
    assert re.search(r"typedef\s+struct\s+str_er_line_crop\s*\{\s*uint64_t\s+pix_off;\s*int32_t\s+width,\s*height;\s*int32_t\s+ax,\s*ay;\s*"
                     r"int32_t\s+ux,\s*uy,\s*vx,\s*vy;\s*\}\s*str_er_line_crop;", txt)
    assert re.search(r"int\s+str_er_set_line_crop\s*\(\s*str_er_ctx\s*\*\s*ctx\s*,\s*int32_t\s+height\s*,\s*int32_t\s+max_width\s*,\s*double\s+pad\s*\)", txt)
    assert re.search(r"const\s+str_er_line_crop\s*\*\s*str_er_result_line_crops\s*\(\s*const\s+str_er_result\s*\*\s*r\s*,\s*int32_t\s*\*\s*n\s*\)", txt)


def test_line_crop_layout_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n'
                   "typedef char size_ok[sizeof(str_er_line_crop) == 40 ? 1 : -1];\n"
                   "typedef char o0[offsetof(str_er_line_crop, pix_off) == 0 ? 1 : -1];\n"
                   "typedef char o1[offsetof(str_er_line_crop, width) == 8 && offsetof(str_er_line_crop, height) == 12 ? 1 : -1];\n"
                   "typedef char o2[offsetof(str_er_line_crop, ax) == 16 && offsetof(str_er_line_crop, ay) == 20 ? 1 : -1];\n"
                   "typedef char o3[offsetof(str_er_line_crop, ux) == 24 && offsetof(str_er_line_crop, uy) == 28 ? 1 : -1];\n"
                   "typedef char o4[offsetof(str_er_line_crop, vx) == 32 && offsetof(str_er_line_crop, vy) == 36 ? 1 : -1];\n"
                   "typedef char fl[STR_ER_WANT_LINE_CROPS == 2048u && STR_ER_WANT_LINE_GLYPHS == 4096u ? 1 : -1];\n"
                   "int main(void) { size_ok a; o0 b; o1 c; o2 d; o3 e; o4 f; fl g;\n"
                   "  const str_er_line_crop *(*h)(const str_er_result *, int32_t *) = str_er_result_line_crops;\n"
                   "  const uint8_t *(*i)(const str_er_result *, uint64_t *) = str_er_result_line_crop_pixels;\n"
                   "  const uint8_t *(*j)(const str_er_result *, uint64_t *) = str_er_result_line_glyph_pixels;\n"
                   "  int (*k)(str_er_ctx *, int32_t, int32_t, double) = str_er_set_line_crop;\n"
                   "  int (*l)(const int32_t *, int32_t, double, int32_t, int32_t, double, str_er_line_crop *) = str_er_line_crop_geometry;\n"
                   "  int (*m)(str_er_ctx *, const uint8_t *, int32_t, int32_t, int64_t, const int32_t *, const int32_t *, const int32_t *,\n"
                   "           const double *, int32_t, uint8_t *, uint64_t, uint64_t *, str_er_line_crop *) = str_er_line_crops;\n"
                   "  (void)a; (void)b; (void)c; (void)d; (void)e; (void)f; (void)g; (void)h; (void)i; (void)j; (void)k; (void)l; (void)m;\n"
                   "  return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_library_exports_the_symbols(S):
    L = S.load_library()
    for name in FUNCS:
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS:
        assert re.search(r"\bT\s+" + name + r"\b", out), name


def test_binding_line_crop_dtype(S):
    import inspect
    assert S.WANT_LINE_CROPS == 2048 and S.WANT_LINE_GLYPHS == 4096
    d = S.LINE_CROP_DTYPE
    assert d.itemsize == 40
    assert [(n, d.fields[n][1]) for n in d.names] == [("pix_off", 0), ("width", 8), ("height", 12), ("ax", 16), ("ay", 20), ("ux", 24),
                                                      ("uy", 28), ("vx", 32), ("vy", 36)]
    assert d["pix_off"] == np.dtype("<u8") and all(d[n] == np.dtype("<i4") for n in d.names[1:])
    for m in ("set_line_crop", "line_crops", "text_detect", "text_detect_list"):
        assert callable(getattr(S.ERFilter, m))
    for m in ("text_detect", "text_detect_list"):
        assert inspect.signature(getattr(S.ERFilter, m)).parameters["want_line_crops"].default is False
    for m in ("line_crop", "line_glyph", "line_crop_batch"):
        assert callable(getattr(S.Result, m))


def test_result_crops_from_hand_made_records(S):
    import importlib
    b = importlib.import_module("scene-text-recognition_amd.binding")
    r = b.Result(np.zeros(0, S.PLANE_DTYPE), np.zeros(0, S.CAND_DTYPE), np.zeros(7), {})
    with pytest.raises(ValueError):
        r.line_crop(0)
    r.line_crops = np.zeros(2, S.LINE_CROP_DTYPE)
    r.line_crops["width"] = [3, 5]
    r.line_crops["height"] = [2, 2]
    r.line_crops["pix_off"] = [0, 8]
    r.line_crop_pixels = np.arange(18, dtype=np.uint8)
    assert r.line_crop(0).tolist() == [[0, 1, 2], [3, 4, 5]]
    assert r.line_crop(1).tolist() == [[8, 9, 10, 11, 12], [13, 14, 15, 16, 17]]
    with pytest.raises(ValueError):
        r.line_glyph(0)
    batch, widths = r.line_crop_batch()
    assert batch.shape == (2, 2, 5) and widths.tolist() == [3, 5]
    assert batch[0].tolist() == [[0, 1, 2, 0, 0], [3, 4, 5, 0, 0]]


# ---- the host geometry ------------------------------------------------------------------------------------------------------------

def _geo(S, boxes, slope, **kw):
    return fields(S.line_crop_geometry(np.asarray(boxes, np.int32), slope, **kw))


def test_geometry_one_box_slope_zero(S):
    box = [(10, 20, 40, 16)]
    g = _geo(S, box, 0.0)
    assert g == geometry(box, 0.0)
    width, height, ax, ay, ux, uy, vx, vy = g
    # the padded union box: pad 2 pixels (0.125 * 16) on every side, 20 x 32 height -> kv = 0.625, width = ceil(44 / 0.625) = 71
    assert height == 32 and width == 71
    assert uy == 0 and vx == 0 and vy == 40960
    assert ux == _llround(65536 * (44 / 71))
    assert ax == _llround(65536 * (8 + 0.5 * 44 / 71 - 0.5)) and ay == _llround(65536 * (18 + 0.3125 - 0.5))
    rec = S.line_crop_geometry(np.asarray(box, np.int32), 0.0)
    assert int(rec["pix_off"]) == 0


@pytest.mark.parametrize("slope", [0.2, -0.2, 3.0, 0.0371])
def test_geometry_slopes(S, slope):
    boxes = [(5, 30, 12, 20), (22, 33, 10, 18), (40, 38, 14, 22), (61, 42, 9, 17)]
    for kw in ({}, {"height": 48, "pad": 0.25}, {"height": 16, "pad": 0.0}):
        assert _geo(S, boxes, slope, **kw) == geometry(boxes, slope, **kw)


@pytest.mark.parametrize("slope", [float("nan"), float("inf"), float("-inf")])
def test_geometry_non_finite_slope_is_zero(S, slope):
    boxes = [(3, 4, 20, 11), (30, 2, 7, 13)]
    assert _geo(S, boxes, slope) == _geo(S, boxes, 0.0) == geometry(boxes, 0.0)


def test_geometry_squeezed_to_max_width(S):
    boxes = [(0, 0, 1900, 10)]
    g = _geo(S, boxes, 0.01, height=32, max_width=64)
    assert g == geometry(boxes, 0.01, height=32, max_width=64)
    assert g[0] == 64 and g[4] > 10 * 65536                    # each output column spans many source pixels
    assert _geo(S, boxes, 0.01, max_width=1)[0] == 1


def test_geometry_bad_arguments(S):
    box = np.asarray([(1, 2, 3, 4)], np.int32)
    for kw in ({"height": 7}, {"height": 257}, {"max_width": 0}, {"max_width": 8193}, {"pad": -0.01}, {"pad": 1.5}, {"pad": float("nan")}):
        with pytest.raises(S.StrErError) as e:
            S.line_crop_geometry(box, 0.0, **kw)
        assert e.value.code == -1, kw
    for bad in (np.zeros((0, 4), np.int32), np.asarray([(1, 2, 0, 4)], np.int32), np.asarray([(1, 2, 3, -1)], np.int32)):
        with pytest.raises(S.StrErError):
            S.line_crop_geometry(bad, 0.0)
    with pytest.raises(S.StrErError):                       # outside 16.16 fixed point
        S.line_crop_geometry(np.asarray([(40000, 0, 10, 10)], np.int32), 0.0)


# ---- the numpy sampler of the GPU tests ---------------------------------------------------------------------------------------------

def test_sampler_identity_map():
    rng = np.random.default_rng(5)
    plane = rng.integers(0, 256, (23, 37), dtype=np.uint8)
    ident = (37, 23, 0, 0, 65536, 0, 0, 65536)
    assert (sample_grey(plane, ident) == plane).all()
    mask = plane > 128
    assert (sample_glyph(mask, ident) == np.where(mask, 255, 0)).all()
    # half a pixel right: the mean of two neighbours, rounded; off the plane: clamped / 0
    half = (36, 23, 32768, 0, 65536, 0, 0, 65536)
    p = plane.astype(np.int64)
    assert (sample_grey(plane, half) == ((p[:, :-1] * 128 + p[:, 1:] * 128) * 256 + 32768) >> 16).all()
    off = (5, 5, -10 * 65536, 0, 65536, 0, 0, 65536)
    assert (sample_grey(plane, off) == plane[:5, :1]).all() and not sample_glyph(mask, off).any()


def test_cpp_example_compiles(S, tmp_path):
    libdir = os.path.dirname(S.lib_path())
    exe = str(tmp_path / "example_line_crops")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(HOST, "example_line_crops.cpp"), "-I", HOST,
                    "-I", os.path.join(ROOT, "include"), "-L", libdir, "-lstr_er_hip", f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    assert os.path.exists(exe)
