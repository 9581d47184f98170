"""CPU checks of the pixel masks (STR_ER_WANT_MASKS, str_er_er_masks): header, struct layout, exports, binding, the reference
flood of the GPU tests against the oracle's |C|, and the C++ example."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
HOST = os.path.join(ROOT, "scene-text-recognition_amd", "host")
FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
FUNCS = ("str_er_result_masks", "str_er_result_mask_bits", "str_er_er_masks")


def test_header_declares_masks():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+STR_ER_WANT_MASKS\s+1024u\b", txt)
    assert re.search(r"#define\s+STR_ER_ABI_VERSION\s+2\b", txt)
    assert re.search(r"typedef\s+struct\s+str_er_mask\s*\{\s*uint64_t\s+word_off;\s*uint32_t\s+pixels;\s*uint32_t\s+pitch_words;\s*\}\s*str_er_mask;", txt)
    assert re.search(r"const\s+str_er_mask\s*\*\s*str_er_result_masks\s*\(\s*const\s+str_er_result\s*\*\s*r\s*,\s*int32_t\s*\*\s*n\s*\)", txt)
    assert re.search(r"const\s+uint32_t\s*\*\s*str_er_result_mask_bits\s*\(\s*const\s+str_er_result\s*\*\s*r\s*,\s*uint64_t\s*\*\s*n_words\s*\)", txt)
    assert re.search(r"int\s+str_er_er_masks\s*\(\s*str_er_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*plane\s*,", txt)


def test_mask_layout_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n'
                   "typedef char size_ok[sizeof(str_er_mask) == 16 ? 1 : -1];\n"
                   "typedef char off_ok[offsetof(str_er_mask, word_off) == 0 ? 1 : -1];\n"
                   "typedef char pix_ok[offsetof(str_er_mask, pixels) == 8 ? 1 : -1];\n"
                   "typedef char pitch_ok[offsetof(str_er_mask, pitch_words) == 12 ? 1 : -1];\n"
                   "typedef char flag_ok[STR_ER_WANT_MASKS == 1024u ? 1 : -1];\n"
                   "typedef int (*masks_fn)(str_er_ctx *, const uint8_t *, int32_t, int32_t, int64_t, const str_er_cand *, int32_t, uint32_t *,\n"
                   "                        uint64_t, uint64_t *, uint32_t *);\n"
                   "int main(void) { size_ok a; off_ok b; pix_ok c; pitch_ok d; flag_ok e; masks_fn f = str_er_er_masks;\n"
                   "  const str_er_mask *(*g)(const str_er_result *, int32_t *) = str_er_result_masks;\n"
                   "  const uint32_t *(*h)(const str_er_result *, uint64_t *) = str_er_result_mask_bits;\n"
                   "  (void)a; (void)b; (void)c; (void)d; (void)e; (void)f; (void)g; (void)h; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_library_exports_the_symbols(S):
    L = S.load_library()
    for name in FUNCS:
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS:
        assert re.search(r"\bT\s+" + name + r"\b", out), name


def test_binding_mask_dtype(S):
    assert S.WANT_MASKS == 1024
    d = S.MASK_DTYPE
    assert d.itemsize == 16 and [(n, d.fields[n][1]) for n in d.names] == [("word_off", 0), ("pixels", 8), ("pitch_words", 12)]
    assert d["word_off"] == np.dtype("<u8") and d["pixels"] == np.dtype("<u4") and d["pitch_words"] == np.dtype("<u4")
    for m in ("er_masks", "text_detect", "text_detect_list"):
        assert callable(getattr(S.ERFilter, m))
    import inspect
    for m in ("text_detect", "text_detect_list"):
        p = inspect.signature(getattr(S.ERFilter, m)).parameters["want_masks"]
        assert p.default is False


def test_result_mask_unpacks_hand_made_words(S):
    b = importlib.import_module("scene-text-recognition_amd.binding")
    cands = np.zeros(3, S.CAND_DTYPE)
    cands["w"] = [3, 33, 64]
    cands["h"] = [2, 2, 1]
    r = b.Result(np.zeros(0, S.PLANE_DTYPE), cands, np.zeros(7), {})
    # mask 0: 3 x 2, rows 0b101 and 0b010 (padding bits of the word left 0); mask 1: 33 x 2, pitch 2; mask 2: 64 x 1
    words = np.array([0b101, 0b010,
                      0x80000001, 0x1, 0x0, 0x0,
                      0xFFFF0000, 0x0000FFFF], np.uint32)
    r.masks = np.zeros(3, S.MASK_DTYPE)
    r.masks["word_off"] = [0, 2, 6]
    r.masks["pitch_words"] = [1, 2, 2]
    r.masks["pixels"] = [3, 3, 32]
    r.mask_bits = words
    m0 = r.mask(0)
    assert m0.dtype == bool and m0.shape == (2, 3)
    assert m0.tolist() == [[True, False, True], [False, True, False]]
    m1 = r.mask(1)
    assert m1.shape == (2, 33) and np.nonzero(m1[0])[0].tolist() == [0, 31, 32] and not m1[1].any()
    m2 = r.mask(2)
    assert m2.shape == (1, 64) and np.nonzero(m2[0])[0].tolist() == list(range(16, 48))
    assert r.mask_pixels.tolist() == [3, 3, 32]
    assert b.Result(np.zeros(0, S.PLANE_DTYPE), cands, np.zeros(7), {}).mask_pixels is None
    with pytest.raises(ValueError):
        b.Result(np.zeros(0, S.PLANE_DTYPE), cands, np.zeros(7), {}).mask(0)


def _flood_count(q, node, w):
    ky, kx = divmod(int(node["key"]), w)
    lab, _ = ndimage.label(q <= int(node["level"]), structure=FOUR)
    return int((lab == lab[ky, kx]).sum()), lab == lab[ky, kx]


@pytest.mark.parametrize("step", [8, 13])
def test_reference_flood_gives_npix(S, oracle, step):
    """The GPU tests' reference: a 4-connected flood of {L <= level} from the key is the node's |C| (oracle npix) with its box."""
    sy = S.synth
    crop = np.load(os.path.join(ROOT, "tests", "golden", "icdar_crops.npz"))["crop1"]
    planes = [oracle.compute_channels(sy.stext_bgr(sy.frame_seed(790), 160, 120))[0],
              oracle.compute_channels(sy.snoise_bgr(sy.frame_seed(791), 48, 40))[1],
              oracle.compute_channels(np.ascontiguousarray(crop))[3]]
    lut = oracle.quant_lut(step)
    for img in planes:
        tree = oracle.tree_extract(img, step=step).nodes
        q = lut[img]
        assert len(tree) > 3
        for t in tree:
            n, m = _flood_count(q, t, img.shape[1])
            assert n == int(t["npix"]) == int(t["area"]) - int(t["nsub"])
            ys, xs = np.nonzero(m)
            assert (xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1) == (int(t["x"]), int(t["y"]), int(t["w"]), int(t["h"]))


def test_cpp_example_compiles(S, tmp_path):
    libdir = os.path.dirname(S.lib_path())
    exe = str(tmp_path / "example_er_masks")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(HOST, "example_er_masks.cpp"), "-I", HOST,
                    "-I", os.path.join(ROOT, "include"), "-L", libdir, "-lstr_er_hip", f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    assert os.path.exists(exe)
