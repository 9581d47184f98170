"""CPU checks of the list entry points (frames of different sizes in one call): header, struct layout, binding, C++ mirror."""
import ctypes as C
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
HOST = os.path.join(ROOT, "scene-text-recognition_amd", "host")


def test_header_declares_the_list_calls():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("str_er_detect_bgr_list", "str_er_detect_planes_list"):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*str_er_ctx\s*\*\s*ctx\s*,\s*const\s+str_er_image_ref\s*\*", txt), name
    assert re.search(r"#define\s+STR_ER_ABI_VERSION\s+2\b", txt)


def test_image_ref_layout_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n'
                   "typedef char size_ok[sizeof(str_er_image_ref) == 24 ? 1 : -1];\n"
                   "typedef char data_ok[offsetof(str_er_image_ref, data) == 0 ? 1 : -1];\n"
                   "typedef char w_ok[offsetof(str_er_image_ref, w) == 8 ? 1 : -1];\n"
                   "typedef char h_ok[offsetof(str_er_image_ref, h) == 12 ? 1 : -1];\n"
                   "typedef char stride_ok[offsetof(str_er_image_ref, stride) == 16 ? 1 : -1];\n"
                   "typedef int (*list_fn)(str_er_ctx *, const str_er_image_ref *, int32_t, int, uint32_t, str_er_result **);\n"
                   "int main(void) { str_er_image_ref r; size_ok a; data_ok b; w_ok c; h_ok d; stride_ok e;\n"
                   "  list_fn f1 = str_er_detect_bgr_list, f2 = str_er_detect_planes_list;\n"
                   "  (void)a; (void)b; (void)c; (void)d; (void)e; (void)f1; (void)f2; r.data = 0; r.w = r.h = 1; r.stride = 3;\n"
                   "  return r.w - 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_binding_image_ref_matches(S):
    b = importlib.import_module("scene-text-recognition_amd.binding")
    R = b.ImageRef
    assert C.sizeof(R) == 24
    assert [(n, getattr(R, n).offset, getattr(R, n).size) for n, _ in R._fields_] == [("data", 0, 8), ("w", 8, 4), ("h", 12, 4), ("stride", 16, 8)]
    for m in ("text_detect_list", "detect_planes_list", "detect_bgr_list_device"):
        assert callable(getattr(S.ERFilter, m))
    L = S.load_library()
    assert hasattr(L, "str_er_detect_bgr_list") and hasattr(L, "str_er_detect_planes_list")


def test_binding_keeps_strided_views():
    import numpy as np
    b = importlib.import_module("scene-text-recognition_amd.binding")
    big = np.zeros((40, 50, 3), np.uint8)
    v = big[3:30, 5:41]
    assert b._row_view(v, 3).ctypes.data == v.ctypes.data          # a row stride: passed as it is
    g = np.zeros((20, 30), np.uint8)[2:, 4:25]
    assert b._row_view(g, 1).ctypes.data == g.ctypes.data
    t = np.zeros((3, 4, 5), np.uint8).transpose(1, 2, 0)             # pixels not interleaved: copied
    assert b._row_view(t[:, :, :3], 3).flags.c_contiguous


def test_host_mirror_batch_compiles(S, tmp_path):
    libdir = os.path.dirname(S.lib_path())
    src = tmp_path / "batch.cpp"
    src.write_text('#include "er_filter_hip.hpp"\nusing namespace str_er_host;\n'
                   "int main() {\n  std::vector<uint8_t> a(3 * 8 * 6), b(3 * 5 * 7);\n"
                   "  std::vector<Image8> frames{Image8(a.data(), 8, 6, 24, 3), Image8(b.data(), 5, 7, 15, 3)};\n"
                   "  std::vector<std::vector<ERTree>> trees; std::vector<ERs> root; std::vector<std::vector<ERs>> pool, strong, weak;\n"
                   "  try { ERFilter f(8, 120, 900000, 2, 0.7, 0.15, 8, 7, 2);\n"
                   "        std::vector<double> t = f.text_detect_batch(frames, trees, root, pool, strong, weak); return t.size() == 7 ? 0 : 1; }\n"
                   "  catch (const std::exception &) { return 2; }\n}\n")
    exe = str(tmp_path / "batch")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", str(src), "-I", HOST, "-I", os.path.join(ROOT, "include"),
                    "-L", libdir, "-lstr_er_hip", f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(HOST, "example_image_batch.cpp"), "-I",
                    os.path.join(ROOT, "include"), "-L", libdir, "-lstr_er_hip", f"-Wl,-rpath,{libdir}", "-o", str(tmp_path / "eib")], check=True)
