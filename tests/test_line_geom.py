"""STR_ER_WANT_LINE_GEOM / str_er_feet_geom on the GPU: the hull, the moments and the oriented box of every footprint, line and frame
line against the reference (line_geom_ref.py, frame_lines_ref.py), every field with ==."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frame_lines_ref as FR
import line_geom_ref as R
from test_frame_lines import GROUPED, ROOT, _crops, _ctx, _same, reference as frame_lines_reference

pytestmark = pytest.mark.gpu
W, H = R.FRAME_W, R.FRAME_H
TABLES = ("line_geoms", "frame_line_geoms", "geom_points")


def _feet(S, items):
    """(x0, y0, bits) footprints as the arguments of feet_geom: LINE_FOOT_DTYPE records and the words back to back."""
    feet = [FR.Foot(x, y, b) if b.size else FR.Foot() for x, y, b in items]
    ft = np.zeros(len(feet), S.LINE_FOOT_DTYPE)
    for t, f in enumerate(feet):
        ft[t]["x"], ft[t]["y"], ft[t]["w"], ft[t]["h"], ft[t]["pixels"] = f.x, f.y, f.w, f.h, f.pixels
    return ft, np.concatenate([f.words() for f in feet] + [np.zeros(0, "<u4")])


def _check_all(geoms, points, refs, names):
    assert len(geoms) == len(refs)
    for g, ref, name in zip(geoms, refs, names):
        msg = R.same(g, points, ref)
        assert msg is None, (name, msg)
    assert len(points) == sum(len(r[3]) for r in refs)            # the hulls back to back, nothing else


# ---- str_er_feet_geom on hand-made footprints ---------------------------------------------------------------------------------------------

def test_feet_geom_shapes(S, cascade_paths):
    shapes = R.shapes()
    refs = {k: R.geom(b, x, y) for k, (x, y, b) in shapes.items()}
    # what the shapes were made for, on the reference alone
    assert refs["pixel_00"][3] == [(0, 0), (1, 0), (1, 1), (0, 1)] and refs["pixel_last"][3][2] == (W, H)
    assert shapes["row_65"][0] == 31 and shapes["row_65"][2].shape == (1, 65) and shapes["column_65"][2].shape == (65, 1)
    x0, _, two = shapes["two_blobs"]
    assert x0 == 33 and two.shape[1] == 70 and not two[3:7].any() and two[1].any() and not two[1, :64].any() and not two[7, :64].any()
    assert len(refs["staircase"][3]) == 6 and refs["sheared_bar"][0]["ey"] != 0
    assert len(refs["disc_40"][3]) == 48 and len(refs["lens_70"][3]) > 128
    assert shapes["tall_1100"][2].shape[0] + 1 > 1024                 # past the rows the kernel keeps in LDS
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=1)
    ft, wd = _feet(S, list(shapes.values()))
    geoms, points = f.feet_geom(W, H, ft, wd)
    _check_all(geoms, points, list(refs.values()), list(shapes))
    # each alone (another slot and another grid), and the C++-style count-only call
    for k, item in shapes.items():
        one_f, one_w = _feet(S, [item])
        g, p = f.feet_geom(W, H, one_f, one_w)
        _check_all(g, p, [refs[k]], [k])
    n = C.c_int32()
    out = np.zeros(len(ft), S.LINE_GEOM_DTYPE)
    assert f.L.str_er_feet_geom(f.h, W, H, ft.ctypes.data, wd.ctypes.data, len(ft), out.ctypes.data, None, 0, C.byref(n)) == 0
    assert n.value == len(points) and out.tobytes() == geoms.tobytes()
    small = np.zeros((3, 2), np.int32)
    assert f.L.str_er_feet_geom(f.h, W, H, ft.ctypes.data, wd.ctypes.data, len(ft), out.ctypes.data, small.ctypes.data, 3, C.byref(n)) == -7
    assert n.value == len(points)
    f.close()


def test_feet_geom_many_empty_and_errors(S, cascade_paths):
    items = R.random_feet(np.random.default_rng(3))
    refs = [R.geom(b, x, y) for x, y, b in items]
    assert len(items) == 200 and refs[17] is R.EMPTY and max(b.shape[1] for _, _, b in items) > 128 and max(b.shape[0] for _, _, b in items) > 64
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=1)
    ft, wd = _feet(S, items)
    geoms, points = f.feet_geom(W, H, ft, wd)
    _check_all(geoms, points, refs, list(range(200)))
    assert int(geoms[17]["count"]) == 0 and int(geoms[17]["edge"]) == -1 and float(geoms[17]["qx"].sum()) == 0.0
    # nothing at all, and only empty footprints
    g, p = f.feet_geom(W, H, ft[:0], wd[:0])
    assert len(g) == 0 and len(p) == 0
    g, p = f.feet_geom(W, H, *_feet(S, [items[17], items[17]]))
    assert len(p) == 0 and [int(v) for v in g["edge"]] == [-1, -1]
    # a foot box 16385 wide: beyond the promise of the moments
    wide_f, wide_w = _feet(S, [(0, 3, np.ones((1, 16385), bool))])
    with pytest.raises(S.StrErError) as e:
        f.feet_geom(20000, H, np.concatenate([ft[:3], wide_f]), np.concatenate([wd[:int(sum(FR.Foot(x, y, b).words().size for x, y, b in items[:3]))], wide_w]))
    assert e.value.code == -7
    ok_f, ok_w = _feet(S, [(0, 3, np.ones((1, 16384), bool))])
    g, p = f.feet_geom(20000, H, ok_f, ok_w)
    _check_all(g, p, [R.geom(np.ones((1, 16384), bool), 0, 3)], ["16384"])
    # malformed input is refused as str_er_link_feet refuses it, the context stays usable
    one, one_w = _feet(S, [(10, 10, np.ones((4, 40), bool))])
    for change in ("leaves", "pixels", "tail", "size"):
        a, b, fw = one.copy(), one_w.copy(), W
        if change == "leaves":
            a[0]["x"] = W - 39
        elif change == "pixels":
            a[0]["pixels"] += 1
        elif change == "tail":
            b[1] |= np.uint32(1 << 8)
        else:
            fw = 65536
        with pytest.raises(S.StrErError) as e:
            f.feet_geom(fw, H, a, b)
        assert e.value.code == -1, change
    geoms2, points2 = f.feet_geom(W, H, ft, wd)
    assert geoms2.tobytes() == geoms.tobytes() and points2.tobytes() == points.tobytes()
    f.close()


# ---- the fused call ---------------------------------------------------------------------------------------------------------------------

def reference(res, sizes):
    """The geometry of every line and frame line of a result that carries its masks (want_masks=True) and frame lines, by the references."""
    feet = frame_lines_reference(res, sizes)[0]
    lines = [R.geom(f.bits, f.x, f.y) for f in feet]
    frame_lines = []
    for g in res.frame_lines:
        mem = [int(t) for t in res.frame_line_members[int(g["first"]):int(g["first"]) + int(g["count"])]]
        frame_lines.append(R.merged([lines[t] for t in mem], lines[int(g["rep"])]))
    return feet, lines, frame_lines


def check(res, ref):
    feet, lines, frame_lines = ref
    assert len(res.line_geoms) == len(lines) == len(res.texts) and len(res.frame_line_geoms) == len(frame_lines) == len(res.frame_lines)
    pts = res.geom_points
    for t, r in enumerate(lines):
        msg = R.same(res.line_geoms[t], pts, r)
        assert msg is None, ("line", t, msg)
        assert res.line_hull(t).tolist() == [list(p) for p in r[3]] and res.line_quad(t).tolist() == [list(p) for p in zip(r[1], r[2])]
    for i, r in enumerate(frame_lines):
        msg = R.same(res.frame_line_geoms[i], pts, r)
        assert msg is None, ("frame line", i, msg)
        assert res.frame_line_hull(i).tolist() == [list(p) for p in r[3]] and res.frame_line_quad(i).tolist() == [list(p) for p in zip(r[1], r[2])]
    assert len(pts) == sum(len(r[3]) for r in lines) + sum(len(r[3]) for r in frame_lines)
    # a frame line's hull is the hull of the union of its members' footprints as well
    for i, g in enumerate(res.frame_lines):
        mem = [int(t) for t in res.frame_line_members[int(g["first"]):int(g["first"]) + int(g["count"])]]
        if len(mem) > 1:
            assert R.hull_of_points(np.concatenate([R.corners(feet[t].bits, feet[t].x, feet[t].y) for t in mem])) == frame_lines[i][3], i


def test_fused_one_frame_and_a_list(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=2, n_pyr_levels=4)
    sy = S.synth
    frame = sy.stext_bgr(sy.frame_seed(2), 640, 480)                 # the frame of test_frame_lines.py::test_threshold
    res = f.text_detect(frame, GROUPED, want_masks=True, want_frame_lines=True, want_line_geom=True)
    ref = reference(res, [(640, 480)])
    assert len(ref[1]) > 0 and any(r[0]["pixels"] > 0 for r in ref[1]) and any(int(g["count"]) > 1 for g in res.frame_lines)
    check(res, ref)
    frames = [frame, sy.stext_bgr(sy.frame_seed(971), 333, 211)]
    lst = f.text_detect_list(frames, GROUPED, want_masks=True, want_frame_lines=True, want_line_geom=True)
    ref = reference(lst, [(640, 480), (333, 211)])
    assert {int(t["frame"]) for t in lst.texts} == {0, 1}
    check(lst, ref)
    # without the masks in the result (the stage makes the members' masks itself), and beside the links
    for kw in ({}, {"want_line_links": True}):
        lean = f.text_detect_list(frames, GROUPED, want_frame_lines=True, want_line_geom=True, **kw)
        for k in TABLES:
            assert getattr(lean, k).tobytes() == getattr(lst, k).tobytes(), (kw, k)
    # a grouped call without lines: empty tables, not an error
    blank = f.text_detect(np.full((120, 160, 3), 128, np.uint8), GROUPED, want_frame_lines=True, want_line_geom=True)
    assert len(blank.texts) == 0 and len(blank.line_geoms) == 0 and len(blank.frame_line_geoms) == 0 and blank.geom_points.shape == (0, 2)
    f.close()


def test_nv12_list_and_the_stream(S, cascade_paths):
    prm = S.Params(max_width=640, max_height=480, max_frames=8, n_pyr_levels=3)
    f = S.ERFilter(params=prm)
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    sy = S.synth
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_GEOM
    frames = _crops()[:2] + [sy.stext_bgr(sy.frame_seed(971), 333, 211), sy.stext_bgr(sy.frame_seed(972), 517, 301)]
    lst = f.text_detect_list(frames, GROUPED, want_frame_lines=True, want_line_geom=True)
    assert len(lst.line_geoms) > 0 and len(lst.geom_points) > 0
    st = S.FrameStream(prm, depth=2)
    st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
    st.submit_copy_list(frames, flags)
    _, a = st.next()
    for k in TABLES:
        assert getattr(a, k).tobytes() == getattr(lst, k).tobytes(), k
    st.close()
    nvf = [sy.stext_bgr(sy.frame_seed(976), 640, 480), sy.stext_bgr(sy.frame_seed(977), 322, 244)]
    nv = [sy.nv12_from_bgr(b) for b in nvf]
    nres = f.text_detect_nv12_list(nv, flags | S.WANT_MASKS)
    assert len(nres.texts) > 0
    check(nres, reference(nres, [(b.shape[1], b.shape[0]) for b in nvf]))
    one = f.text_detect_nv12(nv[0], 640, 480, flags)
    n0 = len(one.texts)
    assert n0 > 0 and nres.line_geoms[:n0].tobytes() == one.line_geoms.tobytes()
    f.close()


def test_line_geom_changes_nothing_else(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=4, n_pyr_levels=2)
    sy = S.synth
    frames = [sy.stext_bgr(sy.frame_seed(2), 640, 480), _crops()[1], sy.snoise_bgr(sy.frame_seed(980), 200, 100)]
    every = (S.WANT_NODES | S.WANT_MASKS | S.WANT_SHAPES | S.WANT_STROKES | S.WANT_LINE_CROPS | S.WANT_LINE_GLYPHS | S.WANT_TEXT_MAP |
             S.WANT_LINE_MAP | S.WANT_LINE_LINKS)
    got = []
    for extra in (0, S.WANT_MASKS, every):
        plain = f.text_detect_list(frames, GROUPED | S.WANT_FRAME_LINES | extra)
        with pytest.raises(ValueError):
            plain.line_geoms
        r = f.text_detect_list(frames, GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_GEOM | extra)
        _same(plain, r)
        for k in ("line_feet", "line_pairs", "frame_lines", "frame_line_members"):
            assert getattr(plain, k).tobytes() == getattr(r, k).tobytes(), k
        if extra & S.WANT_LINE_LINKS:
            for k in ("line_links", "line_tracks", "text_tracks", "text_track_members"):
                assert getattr(plain, k).tobytes() == getattr(r, k).tobytes(), k
        got.append(r)
    for r in got[1:]:
        for k in TABLES:
            assert getattr(r, k).tobytes() == getattr(got[0], k).tobytes(), k
    assert len(got[0].texts) > 0 and len(got[0].frame_line_geoms) > 0
    f.close()


def test_errors(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=320, max_height=240, max_frames=1)
    frame = S.synth.stext_bgr(S.synth.frame_seed(981), 320, 240)
    good = f.text_detect(frame, GROUPED, want_frame_lines=True, want_line_geom=True)

    def usable():
        again = f.text_detect(frame, GROUPED, want_frame_lines=True, want_line_geom=True)
        assert again.line_geoms.tobytes() == good.line_geoms.tobytes() and again.geom_points.tobytes() == good.geom_points.tobytes()

    with pytest.raises(S.StrErError) as e:                           # without STR_ER_WANT_FRAME_LINES
        f.text_detect(frame, GROUPED, want_line_geom=True)
    assert e.value.code == -1 and "STR_ER_WANT_LINE_GEOM" in str(e.value)
    usable()
    planes = f.compute_channels(frame)                               # the per-plane calls
    with pytest.raises(S.StrErError) as e:
        f.detect_planes(planes[:1], S.STAGE_ALL | S.WANT_FRAME_LINES | S.WANT_LINE_GEOM)
    assert e.value.code == -1 and "STR_ER_WANT_LINE_GEOM" in str(e.value)
    usable()
    with pytest.raises(S.StrErError) as e:
        f.detect_planes_list([planes[0], planes[1][:100, :90]], S.STAGE_ALL | S.WANT_FRAME_LINES | S.WANT_LINE_GEOM)
    assert e.value.code == -1
    usable()
    blob = (C.c_char * 16)()                                         # the strip path
    blobs = (C.c_void_p * 1)(C.cast(blob, C.c_void_p))
    sizes = (C.c_int64 * 1)(16)
    rh = C.c_void_p()
    rc = f.L.str_er_strip_merge(f.h, frame.ctypes.data, 320, 240, 960, 0, C.cast(blobs, C.c_void_p), C.cast(sizes, C.c_void_p), 1,
                                S.STAGE_ALL | S.WANT_FRAME_LINES | S.WANT_LINE_GEOM, C.byref(rh))
    assert rc == -1 and b"STR_ER_WANT_LINE_GEOM" in f.L.str_er_last_error(f.h)
    usable()
    f.close()


def test_cpp_example(S, cascade_paths, tmp_path):
    libdir = os.path.dirname(S.lib_path())
    exe = str(tmp_path / "example_line_quads")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "scene-text-recognition_amd", "host", "example_line_quads.cpp"),
                    "-I", os.path.join(ROOT, "include"), "-L", libdir, "-lstr_er_hip", f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    frame = S.synth.stext_bgr(S.synth.frame_seed(2), 640, 480)
    raw = tmp_path / "f.bgr"
    raw.write_bytes(np.ascontiguousarray(frame).tobytes())
    out = subprocess.run([exe, cascade_paths[0], cascade_paths[1], str(raw), "640", "480", "3"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [r.split() for r in out.stdout.splitlines()]
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=1, n_pyr_levels=3)
    res = f.text_detect(frame, GROUPED, want_frame_lines=True, want_line_geom=True)
    assert len(rows) == len(res.frame_lines) > 0
    for i, row in enumerate(rows):
        q = res.frame_line_quad(i)
        assert int(row[0]) == int(res.frame_lines[i]["frame"]) and [float(v) for v in row[1:]] == [float(v) for v in q.reshape(-1)], i
    f.close()
