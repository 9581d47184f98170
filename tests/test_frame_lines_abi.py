"""CPU checks of the frame lines (STR_ER_WANT_FRAME_LINES, str_er_line_feet_regions, str_er_frame_lines_from_pairs): header, struct
layouts, exports, binding, the C++ mirror and example, the stage rules, the host function that joins the duplicates against the numpy
reference, and that reference against a brute-force loop over the pixel rule."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import frame_lines_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
HOST = os.path.join(ROOT, "scene-text-recognition_amd", "host")
CSRC = os.path.join(ROOT, "scene-text-recognition_amd", "csrc")
FUNCS = ("str_er_result_line_feet", "str_er_result_line_pairs", "str_er_result_frame_lines", "str_er_result_frame_line_members",
         "str_er_line_feet_regions", "str_er_frame_lines_from_pairs", "str_er_set_frame_merge")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_flag_structs_and_prototypes():
    txt = _header()
    assert re.search(r"#define\s+STR_ER_WANT_FRAME_LINES\s+\(131072u\)", txt)
    assert re.search(r"#define\s+STR_ER_ABI_VERSION\s+2\b", txt)
    assert re.search(r"typedef\s+struct\s+str_er_line_foot\s*\{\s*int32_t\s+x,\s*y,\s*w,\s*h;\s*uint32_t\s+pixels;\s*int32_t\s+frame_line;\s*\}\s*str_er_line_foot;", txt)
    assert re.search(r"typedef\s+struct\s+str_er_line_pair\s*\{\s*int32_t\s+a,\s*b;\s*uint32_t\s+inter;\s*uint32_t\s+dup;\s*\}\s*str_er_line_pair;", txt)
    assert re.search(r"typedef\s+struct\s+str_er_frame_line\s*\{\s*uint32_t\s+frame;\s*int32_t\s+rep;\s*int32_t\s+first,\s*count;\s*int32_t\s+x,\s*y,\s*w,\s*h;"
                     r"\s*uint32_t\s+pixels;\s*uint32_t\s+levels;\s*\}\s*str_er_frame_line;", txt)
    for ret, name in (("str_er_line_foot", "line_feet"), ("str_er_line_pair", "line_pairs"), ("str_er_frame_line", "frame_lines"),
                      ("int32_t", "frame_line_members")):
        assert re.search(r"const\s+" + ret + r"\s*\*\s*str_er_result_" + name + r"\s*\(\s*const\s+str_er_result\s*\*\s*r\s*,\s*int32_t\s*\*\s*n\s*\)", txt), name
    assert re.search(r"int\s+str_er_set_frame_merge\s*\(\s*str_er_ctx\s*\*\s*ctx\s*,\s*int32_t\s+num\s*,\s*int32_t\s+den\s*\)", txt)
    assert re.search(r"int\s+str_er_line_feet_regions\s*\(\s*str_er_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*plane\s*,", txt)
    assert re.search(r"int\s+str_er_frame_lines_from_pairs\s*\(\s*str_er_line_foot\s*\*\s*feet\s*,", txt)


def test_record_layouts_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n'
                   "#define AT(t, f, o) (offsetof(t, f) == (o))\n"
                   "typedef char foot_ok[sizeof(str_er_line_foot) == 24 && AT(str_er_line_foot, x, 0) && AT(str_er_line_foot, h, 12) &&"
                   " AT(str_er_line_foot, pixels, 16) && AT(str_er_line_foot, frame_line, 20) ? 1 : -1];\n"
                   "typedef char pair_ok[sizeof(str_er_line_pair) == 16 && AT(str_er_line_pair, a, 0) && AT(str_er_line_pair, b, 4) &&"
                   " AT(str_er_line_pair, inter, 8) && AT(str_er_line_pair, dup, 12) ? 1 : -1];\n"
                   "typedef char line_ok[sizeof(str_er_frame_line) == 40 && AT(str_er_frame_line, frame, 0) && AT(str_er_frame_line, rep, 4) &&"
                   " AT(str_er_frame_line, first, 8) && AT(str_er_frame_line, count, 12) && AT(str_er_frame_line, x, 16) &&"
                   " AT(str_er_frame_line, h, 28) && AT(str_er_frame_line, pixels, 32) && AT(str_er_frame_line, levels, 36) ? 1 : -1];\n"
                   "typedef char fl[STR_ER_WANT_FRAME_LINES == 131072u && STR_ER_ABI_VERSION == 2 ? 1 : -1];\n"
                   "typedef int (*feet_fn)(str_er_ctx *, const uint8_t *, int32_t, int32_t, int64_t, const str_er_cand *, const int32_t *, int32_t,"
                   " int32_t, int32_t, int32_t, str_er_line_foot *, uint32_t *, uint64_t, uint64_t *, str_er_line_pair *, int32_t, int32_t *);\n"
                   "typedef int (*join_fn)(str_er_line_foot *, const uint32_t *, const uint8_t *, int32_t, str_er_line_pair *, int32_t, int32_t,"
                   " int32_t, str_er_frame_line *, int32_t, int32_t *, int32_t *);\n"
                   "int main(void) { foot_ok a; pair_ok b; line_ok c; fl d; feet_fn f = str_er_line_feet_regions; join_fn j = str_er_frame_lines_from_pairs;\n"
                   "  int (*m)(str_er_ctx *, int32_t, int32_t) = str_er_set_frame_merge;\n"
                   "  const str_er_line_foot *(*g)(const str_er_result *, int32_t *) = str_er_result_line_feet;\n"
                   "  const str_er_line_pair *(*p)(const str_er_result *, int32_t *) = str_er_result_line_pairs;\n"
                   "  const str_er_frame_line *(*q)(const str_er_result *, int32_t *) = str_er_result_frame_lines;\n"
                   "  const int32_t *(*r)(const str_er_result *, int32_t *) = str_er_result_frame_line_members;\n"
                   "  (void)a; (void)b; (void)c; (void)d; (void)f; (void)j; (void)m; (void)g; (void)p; (void)q; (void)r; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_library_exports_the_symbols(S):
    L = S.load_library()
    for name in FUNCS:
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS:
        assert re.search(r"\bT\s+" + name + r"\b", out), name


def test_binding_constants_dtypes_and_keywords(S):
    assert S.WANT_FRAME_LINES == 131072
    for d, size, offs in ((S.LINE_FOOT_DTYPE, 24, [("x", 0), ("y", 4), ("w", 8), ("h", 12), ("pixels", 16), ("frame_line", 20)]),
                          (S.LINE_PAIR_DTYPE, 16, [("a", 0), ("b", 4), ("inter", 8), ("dup", 12)]),
                          (S.FRAME_LINE_DTYPE, 40, [("frame", 0), ("rep", 4), ("first", 8), ("count", 12), ("x", 16), ("y", 20), ("w", 24), ("h", 28),
                                                    ("pixels", 32), ("levels", 36)])):
        assert d.itemsize == size and [(n, d.fields[n][1]) for n in d.names] == offs
    for m in ("text_detect", "text_detect_list"):
        assert inspect.signature(getattr(S.ERFilter, m)).parameters["want_frame_lines"].default is False
    binding = __import__("importlib").import_module("scene-text-recognition_amd.binding")
    assert binding._want_flags(frame_lines=True) == 131072 and binding._want_flags() == 0
    assert binding._want_flags(frame_lines=True, masks=True, line_map=True) == 131072 | 1024 | 32768
    for m in ("line_feet_regions", "set_frame_merge"):
        assert callable(getattr(S.ERFilter, m))
    assert callable(S.frame_lines_from_pairs)


def test_result_accessors_without_the_flag(S):
    r = S.Result.__new__(S.Result)
    r._line_feet = r._line_pairs = r._frame_lines = r._frame_line_members = None
    for name in ("line_feet", "line_pairs", "frame_lines", "frame_line_members"):
        with pytest.raises(ValueError):
            getattr(r, name)
    r._line_feet = np.zeros(0, S.LINE_FOOT_DTYPE)
    assert len(r.line_feet) == 0


def test_cpp_mirror_and_example_compile(tmp_path):
    for src in ("example_frame_lines.cpp", "example_text_map.cpp"):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), os.path.join(HOST, src)],
                       check=True)


def test_stage_rules_of_the_flag(tmp_path):
    exe = str(tmp_path / "frame_lines_rules_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "frame_lines_rules_check.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith(" 0 wrong")


# ---- str_er_frame_lines_from_pairs against the reference ---------------------------------------------------------------------------------

def _join(S, boxes, pixels, frames, pyr, pairs, num=1, den=2):
    feet = np.zeros(len(pixels), S.LINE_FOOT_DTYPE)
    for t, (b, p) in enumerate(zip(boxes, pixels)):
        feet[t]["x"], feet[t]["y"], feet[t]["w"], feet[t]["h"], feet[t]["pixels"] = b[0], b[1], b[2], b[3], p
    pr = np.zeros(len(pairs), S.LINE_PAIR_DTYPE)
    for k, (a, b, i) in enumerate(pairs):
        pr[k]["a"], pr[k]["b"], pr[k]["inter"] = a, b, i
    return S.frame_lines_from_pairs(feet, frames, pyr, pr, num, den)


def _agree(S, boxes, pixels, frames, pyr, pairs, num=1, den=2):
    ft, pr, fl, mem = _join(S, boxes, pixels, frames, pyr, pairs, num, den)
    dup, frame_line, lines, members = R.frame_lines(boxes, pixels, frames, pyr, pairs, num, den)
    assert [int(d) for d in pr["dup"]] == dup
    assert [int(v) for v in ft["frame_line"]] == frame_line
    assert [{k: int(g[k]) for k in g.dtype.names} for g in fl] == lines
    assert [int(m) for m in mem] == members
    return dup, frame_line, lines


def test_from_pairs_random_cases(S):
    rng = np.random.default_rng(20)
    merged = 0
    for case in range(240):
        n_frames = int(rng.integers(1, 5))
        n = int(rng.integers(0, 40))
        frames = sorted(int(v) for v in rng.integers(0, n_frames, n)) if case % 3 else [int(v) for v in rng.integers(0, n_frames, n)]
        pyr = [int(v) for v in rng.integers(0, 8, n)]
        pixels = [int(v) for v in rng.choice([0, 1, 7, 50, 50, 200, 4000, 2 ** 31], n)]
        boxes = [(int(rng.integers(0, 1900)), int(rng.integers(0, 1000)), int(rng.integers(1, 300)), int(rng.integers(1, 80))) if p else (0, 0, 0, 0)
                 for p in pixels]
        pairs = []
        for a in range(n):
            for b in range(a + 1, n):
                if frames[a] == frames[b] and pixels[a] and pixels[b] and rng.random() < 0.25:
                    m = min(pixels[a], pixels[b])
                    pairs.append((a, b, int(rng.choice([1, max(1, m // 2), max(1, m - 1), m]))))
        num, den = [(1, 2), (1, 1), (1, 50), (3, 4), (65535, 65535), (1, 65535)][case % 6]
        dup, _, lines = _agree(S, boxes, pixels, frames, pyr, pairs, num, den)
        merged += sum(g["count"] > 1 for g in lines)
    assert merged > 50


def test_from_pairs_chains_boundary_ties_and_errors(S):
    box = (0, 0, 10, 10)
    # a ~ b ~ c, a and c without a common pixel: one frame line
    dup, fl, lines = _agree(S, [box] * 3, [100, 100, 100], [0, 0, 0], [0, 1, 2], [(0, 1, 80), (1, 2, 80)])
    assert dup == [1, 1] and fl == [0, 0, 0] and lines[0]["levels"] == 7 and lines[0]["rep"] == 0
    # ... and with a, c a pair that is no duplicate
    dup, fl, _ = _agree(S, [box] * 3, [100, 100, 100], [0, 0, 0], [0, 1, 2], [(0, 1, 80), (0, 2, 1), (1, 2, 80)])
    assert dup == [1, 0, 1] and fl == [0, 0, 0]
    # the boundary: inter * den == num * union is a duplicate, one pixel less is not
    for num, den in ((1, 2), (1, 3), (2, 3), (1, 1), (7, 50)):
        for pa, pb in ((300, 300), (150, 450), (1000, 50 * den)):
            for k in range(1, min(pa, pb) + 1):
                exact = k * den == num * (pa + pb - k)
                if exact or (k + 1) * den == num * (pa + pb - k - 1):
                    dup, _, _ = _agree(S, [box] * 2, [pa, pb], [0, 0], [0, 0], [(0, 1, k)], num, den)
                    assert dup == [1 if exact else 0], (num, den, pa, pb, k)
    dup, _, _ = _agree(S, [box] * 2, [300, 300], [0, 0], [0, 0], [(0, 1, 200)], 1, 2)       # 200 * 2 == 400
    assert dup == [1]
    dup, _, _ = _agree(S, [box] * 2, [300, 300], [0, 0], [0, 0], [(0, 1, 199)], 1, 2)
    assert dup == [0]
    # 64-bit products: 2^31 pixels at den = 65535
    dup, _, _ = _agree(S, [box] * 2, [2 ** 31, 2 ** 31], [0, 0], [0, 0], [(0, 1, 2 ** 31)], 65535, 65535)
    assert dup == [1]
    # representative: most pixels, ties to the smallest line
    _, _, lines = _agree(S, [box] * 3, [90, 100, 100], [0, 0, 0], [3, 3, 4], [(0, 1, 85), (1, 2, 95)])
    assert lines[0]["rep"] == 1 and lines[0]["pixels"] == 100 and lines[0]["levels"] == 0x18
    # order: by frame, then by smallest member, whatever the order of the lines' frames
    _, fl, lines = _agree(S, [box] * 4, [10, 10, 10, 10], [1, 0, 1, 0], [0, 0, 0, 0], [(0, 2, 10)])
    assert [g["frame"] for g in lines] == [0, 0, 1] and fl == [2, 0, 2, 1]
    # errors
    for pairs in ([(0, 1, 5)], [(1, 1, 5)], [(2, 1, 5)], [(0, 4, 5)], [(-1, 2, 5)], [(0, 2, 0)], [(0, 2, 11)]):
        with pytest.raises(S.StrErError) as e:
            _join(S, [box] * 4, [10, 10, 10, 10], [1, 0, 1, 0], [0, 0, 0, 0], pairs)
        assert e.value.code == -1, pairs
    for num, den in ((0, 1), (2, 1), (1, 65536)):
        with pytest.raises(S.StrErError):
            _join(S, [box], [10], [0], [0], [], num, den)
    ft, pr, fl, mem = _join(S, [], [], [], [], [])
    assert len(ft) == len(pr) == len(fl) == len(mem) == 0


# ---- the reference itself ----------------------------------------------------------------------------------------------------------------

def test_reference_footprint_matches_brute_force():
    rng = np.random.default_rng(3)
    for W, H, pw, ph in ((23, 17, 23, 17), (40, 31, 13, 9), (11, 7, 37, 29), (64, 5, 9, 5)):
        lines = []
        for _ in range(5):
            mem = []
            for _ in range(int(rng.integers(1, 4))):
                w, h = int(rng.integers(1, pw + 1)), int(rng.integers(1, ph + 1))
                x, y = int(rng.integers(0, pw - w + 1)), int(rng.integers(0, ph - h + 1))
                mem.append((pw, ph, x, y, rng.random((h, w)) < 0.4))
            lines.append(mem)
        lines.append([(pw, ph, 0, 0, np.zeros((1, 1), bool))])          # an empty footprint
        feet = [R.footprint(W, H, m) for m in lines]
        full = [R.brute_footprint(W, H, m) for m in lines]
        for f, b in zip(feet, full):
            assert f.pixels == int(b.sum())
            if f.pixels:
                ys, xs = np.nonzero(b)
                assert (f.x, f.y, f.w, f.h) == (xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1)
                assert (b[f.y:f.y + f.h, f.x:f.x + f.w] == f.bits).all()
                unpacked = np.unpackbits(f.words().view(np.uint8).reshape(f.h, -1), axis=1, bitorder="little")[:, :f.w].astype(bool)
                assert (unpacked == f.bits).all()
            else:
                assert (f.x, f.y, f.w, f.h) == (0, 0, 0, 0)
        for a in range(len(feet)):
            for b in range(a + 1, len(feet)):
                assert R.inter(feet[a], feet[b]) == int((full[a] & full[b]).sum())
        assert feet[-1].pixels == 0
