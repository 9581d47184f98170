#!/usr/bin/env python3
"""Build libstr_er_hip.so (gfx950) in-tree with hipcc.

    python scene-text-recognition_amd/build.py [--force]

hipcc cross-compiles without a GPU.  The library is written for MI355X (gfx950) only.
-ffp-contract=off keeps the resize coefficient arithmetic identical to the host statement
of cv::resize (no fused multiply-add where the reference has a separate multiply and add).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "lib", "libstr_er_hip.so")
SOURCES = ["er_kernels.hip", "ocr_kernels.hip", "word_match_kernels.hip", "word_decode_kernels.hip", "word_margin_kernels.hip", "line_decode_kernels.hip", "line_margin_kernels.hip", "run_split_kernels.hip", "lattice_decode_kernels.hip", "line_lattice_kernels.hip", "lattice_margin_kernels.hip", "lattice_match_kernels.hip", "lattice_track_kernels.hip", "lattice_track_decode_kernels.hip", "track_match_kernels.hip", "track_decode_kernels.hip", "track_pool_kernels.hip", "decode_pool_kernels.hip", "lattice_decode_pool_kernels.hip", "track_kernels.hip", "er_group.cpp", "flood_order.cpp", "gather.cpp", "str_er_api.cpp", "api_models.cpp", "api_strips.cpp", "api_stages.cpp", "api_line_crops.cpp", "api_text_map.cpp", "api_frame_lines.cpp", "api_run_read.cpp", "api_word_match.cpp", "api_word_decode.cpp", "api_word_margin.cpp", "api_line_decode.cpp", "api_line_margin.cpp", "api_run_split.cpp", "api_lattice_decode.cpp", "api_line_lattice.cpp", "api_lattice_margin.cpp", "api_lattice_match.cpp", "api_lattice_track.cpp", "api_lattice_track_decode.cpp", "api_track_read.cpp", "api_track_decode.cpp", "api_track_pool.cpp", "lines_host.cpp", "words_host.cpp", "stream_api.cpp"]
DEPS = SOURCES + ["er_planes.inl", "er_pyr_level.inl", "resize_tile_body.inl", "ycrcb_quad_body.inl", "nv12_quad_body.inl", "er_tile_tree.inl", "er_tile_tree2.inl", "tile2_body.h", "er_tree_passes.inl", "er_nms.inl", "er_classify.inl", "er_masks.inl", "er_line_crops.inl", "er_text_map.inl", "er_frame_lines.inl", "er_kernels.h", "ocr_kernels.h", "word_match_kernels.h", "word_match_device.h", "word_match_rules.h", "track_match_kernels.h", "track_match_device.h", "track_read_rules.h", "track_decode_kernels.h", "track_decode_rules.h", "track_pool_kernels.h", "track_pool_rules.h", "decode_pool_kernels.h", "decode_pool_device.h", "decode_pool_rules.h", "lattice_decode_pool_kernels.h", "lattice_decode_pool_rules.h", "word_decode_kernels.h", "word_decode_device.h", "word_decode_rules.h", "word_margin_kernels.h", "word_margin_rules.h", "line_decode_kernels.h", "line_decode_rules.h", "line_margin_kernels.h", "line_margin_rules.h", "word_margin_device.h", "lattice_decode_kernels.h", "lattice_decode_rules.h", "line_lattice_kernels.h", "line_lattice_rules.h", "lattice_margin_kernels.h", "lattice_margin_rules.h", "lattice_match_kernels.h", "lattice_match_device.h", "lattice_match_rules.h", "lattice_track_kernels.h", "lattice_track_device.h", "lattice_track_rules.h", "lattice_track_decode_kernels.h", "lattice_track_decode_rules.h", "run_split_kernels.h", "run_split_rules.h", "ocr_device.h", "svm_tables.h", "str_er_ctx.h", "stage_rules.h", "read_plan.h", "frame_rules.h", "track_kernels.h", "er_device.h", "er_group.h", "flood_order.h", "er_types.h", os.path.join("..", "..", "include", "str_er.h")]
EXTRA = os.environ.get("STR_ER_EXTRA_FLAGS", "").split()
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-Wall", "-Wno-unused-function", "-Wno-unused-result", "-Wno-bitwise-instead-of-logical"]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.sep not in cand or os.path.exists(cand)):
            return cand
    return "hipcc"


def needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(os.path.join(CSRC, d)) > t for d in DEPS) or os.path.getmtime(__file__) > t


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    objs = []
    for src in SOURCES:
        obj = os.path.join(HERE, "lib", os.path.splitext(src)[0] + ".o")
        cmd = [hipcc(), *FLAGS, *EXTRA, "-x", "hip", "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        objs.append(obj)
    cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs, "-ldl", "-lpthread"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
