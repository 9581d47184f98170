"""CPU checks of the frame maps (STR_ER_WANT_TEXT_MAP / _LINE_MAP, str_er_text_map_regions): header, struct layout, exports, binding,
the C++ mirror and example, and the numpy reference rasteriser of the GPU tests against a brute-force loop over the pixel rule."""
import inspect
import os
import re
import subprocess

import numpy as np

from text_map_ref import Raster, brute, samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
HOST = os.path.join(ROOT, "scene-text-recognition_amd", "host")
FUNCS = ("str_er_result_frame_maps", "str_er_result_text_map_pixels", "str_er_result_line_map_ids", "str_er_text_map_regions")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_flags_and_struct():
    txt = _header()
    assert re.search(r"#define\s+STR_ER_WANT_TEXT_MAP\s+\(16384u\)", txt)
    assert re.search(r"#define\s+STR_ER_WANT_LINE_MAP\s+\(32768u\)", txt)
    assert re.search(r"#define\s+STR_ER_ABI_VERSION\s+2\b", txt)
    for name, v in (("STRONG", 1), ("WEAK", 2), ("LINE", 4), ("OCR", 8)):
        assert re.search(r"#define\s+STR_ER_TEXT_MAP_" + name + r"\s+" + str(v) + r"u\b", txt), name
    assert re.search(r"typedef\s+struct\s+str_er_frame_map\s*\{\s*uint64_t\s+off;\s*int32_t\s+width,\s*height;\s*\}\s*str_er_frame_map;", txt)
    assert re.search(r"const\s+str_er_frame_map\s*\*\s*str_er_result_frame_maps\s*\(\s*const\s+str_er_result\s*\*\s*r\s*,\s*int32_t\s*\*\s*n\s*\)", txt)
    assert re.search(r"const\s+uint8_t\s*\*\s*str_er_result_text_map_pixels\s*\(\s*const\s+str_er_result\s*\*\s*r\s*,\s*uint64_t\s*\*\s*n_bytes\s*\)", txt)
    assert re.search(r"const\s+int32_t\s*\*\s*str_er_result_line_map_ids\s*\(\s*const\s+str_er_result\s*\*\s*r\s*,\s*uint64_t\s*\*\s*n\s*\)", txt)
    assert re.search(r"int\s+str_er_text_map_regions\s*\(\s*str_er_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*plane\s*,\s*int32_t\s+w\s*,\s*int32_t\s+h\s*,"
                     r"\s*int64_t\s+stride\s*,\s*const\s+str_er_cand\s*\*\s*regions\s*,\s*const\s+uint8_t\s*\*\s*values\s*,\s*const\s+int32_t\s*\*\s*ids\s*,"
                     r"\s*int32_t\s+n\s*,\s*int32_t\s+out_w\s*,\s*int32_t\s+out_h\s*,\s*uint8_t\s*\*\s*out_map\s*,\s*int32_t\s*\*\s*out_ids\s*\)", txt)


def test_frame_map_layout_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n'
                   "typedef char size_ok[sizeof(str_er_frame_map) == 16 ? 1 : -1];\n"
                   "typedef char off_ok[offsetof(str_er_frame_map, off) == 0 && offsetof(str_er_frame_map, width) == 8 &&"
                   " offsetof(str_er_frame_map, height) == 12 ? 1 : -1];\n"
                   "typedef char fl[STR_ER_WANT_TEXT_MAP == 16384u && STR_ER_WANT_LINE_MAP == 32768u && STR_ER_TEXT_MAP_OCR == 8u ? 1 : -1];\n"
                   "typedef int (*map_fn)(str_er_ctx *, const uint8_t *, int32_t, int32_t, int64_t, const str_er_cand *, const uint8_t *,"
                   " const int32_t *, int32_t, int32_t, int32_t, uint8_t *, int32_t *);\n"
                   "int main(void) { size_ok a; off_ok b; fl c; map_fn f = str_er_text_map_regions;\n"
                   "  const str_er_frame_map *(*g)(const str_er_result *, int32_t *) = str_er_result_frame_maps;\n"
                   "  const uint8_t *(*p)(const str_er_result *, uint64_t *) = str_er_result_text_map_pixels;\n"
                   "  const int32_t *(*q)(const str_er_result *, uint64_t *) = str_er_result_line_map_ids;\n"
                   "  (void)a; (void)b; (void)c; (void)f; (void)g; (void)p; (void)q; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_library_exports_the_symbols(S):
    L = S.load_library()
    for name in FUNCS:
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS:
        assert re.search(r"\bT\s+" + name + r"\b", out), name


def test_binding_constants_dtype_and_keywords(S):
    assert (S.WANT_TEXT_MAP, S.WANT_LINE_MAP) == (16384, 32768)
    assert (S.TEXT_MAP_STRONG, S.TEXT_MAP_WEAK, S.TEXT_MAP_LINE, S.TEXT_MAP_OCR) == (1, 2, 4, 8)
    d = S.FRAME_MAP_DTYPE
    assert d.itemsize == 16 and [(n, d.fields[n][1]) for n in d.names] == [("off", 0), ("width", 8), ("height", 12)]
    assert d["off"] == np.dtype("<u8") and d["width"] == np.dtype("<i4")
    for m in ("text_detect", "text_detect_list"):
        ps = inspect.signature(getattr(S.ERFilter, m)).parameters
        assert ps["want_text_map"].default is False and ps["want_line_map"].default is False
    assert hasattr(S.ERFilter, "text_map_regions")
    for m in ("text_map", "line_map"):
        assert callable(getattr(S.Result, m))


def test_result_map_accessors_without_the_flags(S):
    r = S.Result.__new__(S.Result)
    r.frame_maps = r.text_map_pixels = r.line_map_ids = None
    for m in ("text_map", "line_map"):
        try:
            getattr(r, m)(0)
        except ValueError:
            continue
        raise AssertionError(m + " without its flag must raise ValueError")


def test_cpp_mirror_and_example_compile(S, tmp_path):
    txt = open(os.path.join(HOST, "er_filter_hip.hpp")).read()
    assert "text_map_regions(const Image8 &plane, const ERs &ers" in txt and "frame_maps(const str_er_result *r)" in txt
    libdir = os.path.dirname(S.lib_path())
    exe = str(tmp_path / "example_text_map")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(HOST, "example_text_map.cpp"), "-I", HOST,
                    "-I", os.path.join(ROOT, "include"), "-L", libdir, "-lstr_er_hip", f"-Wl,-rpath,{libdir}", "-o", exe], check=True)


# ---- the reference rasteriser ---------------------------------------------------------------------------------------------------------

def test_samples_identity_and_inverse():
    for n in (1, 2, 7, 64, 1920):
        assert (samples(n, n) == np.arange(n)).all()                   # level 0: the identity
    for W, wp in ((1920, 1358), (1920, 240), (7, 3), (5, 11), (3, 8), (1, 5)):
        xs = samples(W, wp)
        assert (np.diff(xs) >= 0).all() and xs.min() >= 0 and xs.max() < wp
        for a in range(wp + 1):            # the host's pre-image: the first x with xs >= a is ceil((2 a W - wp) / (2 wp)), clamped to [0, W]
            num, den = 2 * a * W - wp, 2 * wp
            first = 0 if num <= 0 else min(W, -(-num // den))
            assert first == int(np.searchsorted(xs, a, "left")), (W, wp, a)


def test_raster_matches_brute_force():
    rng = np.random.default_rng(7)
    for case in range(40):
        W, H = int(rng.integers(1, 23)), int(rng.integers(1, 19))
        regions = []
        for _ in range(int(rng.integers(1, 7))):
            pw = int(rng.integers(1, 2 * W + 3))           # below, equal to and above W: downsampled and upsampled levels
            ph = int(rng.integers(1, 2 * H + 3))
            x, y = int(rng.integers(0, pw)), int(rng.integers(0, ph))
            w, h = int(rng.integers(1, pw - x + 1)), int(rng.integers(1, ph - y + 1))
            mask = rng.random((h, w)) < 0.6
            value = int(rng.choice([1, 2, 4, 8, 5, 12]))
            ident = None if rng.random() < 0.3 else int(rng.integers(0, 9))
            regions.append((pw, ph, x, y, mask, value, ident))
        R = Raster(W, H)
        for g in regions:
            R.add(*g)
        m, ids = brute(W, H, regions)
        assert (R.map == m).all(), case
        assert (R.id_map() == ids).all(), case
