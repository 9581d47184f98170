"""Line crops on the GPU (STR_ER_WANT_LINE_CROPS / _GLYPHS, str_er_line_crops): every record against the numpy geometry of the
contract, every grey byte against the numpy sampler on the Y plane of its (frame, pyr), every glyph byte against the nearest sample of
the union of the member masks; nothing else of a call changed by the flags; lists, NV12, the stream and device frames against one
call per frame; the crop settings; hand-made geometry at the kernel's own edges; errors; the single-stage call against the fused one;
the C++ example."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_spec = importlib.util.spec_from_file_location("line_crops_ref", os.path.join(ROOT, "tests", "test_line_crops_abi.py"))
REF = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REF)
GROUPED = 7 | 32 | 64            # STAGE_ALL | STAGE_TRACK | STAGE_GROUP


def _crops():
    z = np.load(os.path.join(GOLDEN, "icdar_crops.npz"))
    return [np.ascontiguousarray(z[k]) for k in sorted(z.files)]


def _ctx(S, cascade_paths, **kw):
    f = S.ERFilter(params=S.Params(**kw))
    f.load_cascade(0, cascade_paths[0])
    f.load_cascade(1, cascade_paths[1])
    return f


def _boxes(res, t):
    tx = res.texts[t]
    m = res.text_ers[int(tx["first"]):int(tx["first"]) + int(tx["count"])]
    gb = res.group_bounds[m]
    return np.stack([gb["x"], gb["y"], gb["w"], gb["h"]], axis=1).astype(np.int64), m


def check_crops(res, y_of, height=32, max_width=1024, pad=0.125, union_of=None):
    """Every line of res: geometry within 1 fixed-point unit of the numpy formula, the layout, grey bytes == the numpy sampler on
    y_of(frame, pyr); with union_of(frame, pyr, members) also the glyph bytes.  Returns the number of lines."""
    assert res.line_crops is not None and len(res.line_crops) == len(res.texts)
    off = 0
    for t, rec in enumerate(res.line_crops):
        boxes, members = _boxes(res, t)
        exp = REF.geometry(boxes, float(res.texts[t]["slope"]), height, max_width, pad)
        got = REF.fields(rec)
        assert got[:2] == exp[:2], t
        assert all(abs(a - b) <= 1 for a, b in zip(got[2:], exp[2:])), (t, got, exp)
        assert int(rec["pix_off"]) == off and off % 4 == 0
        off += (got[0] * got[1] + 3) // 4 * 4
        fr, pyr = int(res.texts[t]["frame"]), int(res.texts[t]["pyr"])
        crop = res.line_crop(t)
        assert crop.shape == (height, got[0])
        assert (crop == REF.sample_grey(y_of(fr, pyr), got)).all(), t
        if union_of is not None:
            assert (res.line_glyph(t) == REF.sample_glyph(union_of(fr, pyr, members), got)).all(), t
    assert off == len(res.line_crop_pixels)
    return len(res.line_crops)


def mask_union(res, y_of):
    """union_of for check_crops from the WANT_MASKS output of the same call: each member's mask over its candidate's box."""
    def union(fr, pyr, members):
        u = np.zeros(y_of(fr, pyr).shape, bool)
        for i in set(int(k) for k in members):
            c = res.cands[i]
            x, y, w, h = int(c["x"]), int(c["y"]), int(c["w"]), int(c["h"])
            u[y:y + h, x:x + w] |= res.mask(i)
        return u
    return union


def test_fused_crops_icdar_and_glyphs(S, cascade_paths, oracle):
    frames = _crops() + [S.synth.stext_bgr(S.synth.frame_seed(2), 640, 480)]
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=len(frames))
    res = f.text_detect_list(frames, GROUPED, want_masks=True, want_line_crops="glyphs")
    ys = [oracle.compute_channels(fr)[0] for fr in frames]
    y_of = lambda fr, pyr: ys[fr]                                   # noqa: E731
    assert check_crops(res, y_of, union_of=mask_union(res, y_of)) > 0
    # the glyph crops do not depend on WANT_MASKS (the masks are then made for the members alone)
    res2 = f.text_detect_list(frames, GROUPED, want_line_crops="glyphs")
    assert res2.masks is None
    assert res2.line_crops.tobytes() == res.line_crops.tobytes()
    assert res2.line_crop_pixels.tobytes() == res.line_crop_pixels.tobytes()
    assert res2.line_glyph_pixels.tobytes() == res.line_glyph_pixels.tobytes()
    assert res.line_glyph_pixels.any()
    f.close()


def test_fused_crops_pyramid_1080p(S, cascade_paths, oracle):
    L = 8
    f = _ctx(S, cascade_paths, max_width=1920, max_height=1080, max_frames=2, n_pyr_levels=L, channel_mask=0x07)
    sy = S.synth
    frames = np.stack([sy.stext_bgr(sy.frame_seed(810 + k), 1920, 1080) for k in range(2)])
    res = f.text_detect(frames, GROUPED | S.GROUP_INNER_SUP, want_masks=True, want_line_crops="glyphs")
    pyr = [oracle.pyramid(oracle.compute_channels(fr)[0], L) for fr in frames]
    y_of = lambda fr, p: pyr[fr][p]                                 # noqa: E731
    n = check_crops(res, y_of, union_of=mask_union(res, y_of))
    assert n > 0
    f.close()


FIELDS = ("info", "cands", "tracks", "texts", "text_ers", "group_bounds", "group_all", "masks", "mask_bits")


def test_flags_change_nothing_else(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=4)
    sy = S.synth
    frames = [sy.stext_bgr(sy.frame_seed(2), 640, 480), _crops()[1], sy.snoise_bgr(sy.frame_seed(821), 200, 100)]
    for extra in (0, S.WANT_MASKS | S.WANT_NODES):
        plain = f.text_detect_list(frames, GROUPED | extra)
        crops = f.text_detect_list(frames, GROUPED | extra | S.WANT_LINE_CROPS)
        glyphs = f.text_detect_list(frames, GROUPED | extra | S.WANT_LINE_CROPS | S.WANT_LINE_GLYPHS)
        assert plain.line_crops is None and crops.line_glyph_pixels is None and glyphs.line_glyph_pixels is not None
        for other in (crops, glyphs):
            for k in FIELDS:
                x, y = getattr(plain, k), getattr(other, k)
                assert (x is None) == (y is None), k
                if x is not None:
                    assert x.tobytes() == y.tobytes(), k
            for pa, pb in zip(plain.planes, other.planes):
                assert (pa.nodes is None) == (pb.nodes is None)
                if pa.nodes is not None:
                    assert pa.nodes.tobytes() == pb.nodes.tobytes()
        assert crops.line_crop_pixels.tobytes() == glyphs.line_crop_pixels.tobytes()
        assert len(plain.texts) > 0
    f.close()


def _frame_crops(res, i):
    """(records without pix_off, grey bytes, glyph bytes) of frame i's lines, in line order."""
    sel = np.nonzero(res.texts["frame"] == i)[0]
    recs = [REF.fields(res.line_crops[t]) for t in sel]
    grey = b"".join(res.line_crop(int(t)).tobytes() for t in sel)
    glyph = b"".join(res.line_glyph(int(t)).tobytes() for t in sel) if res.line_glyph_pixels is not None else None
    return recs, grey, glyph


def _place(buf, frames, bpp=3, rows_of=None):
    layout, at = [], 0
    for k, fr in enumerate(frames):
        rows, w = fr.shape[0], fr.shape[1]
        row = bpp * w
        stride = row + 3 + 2 * k
        at += 1 + k
        for y in range(rows):
            buf[at + y * stride:at + y * stride + row] = fr[y].reshape(-1)
        layout.append((at, w, rows_of(rows) if rows_of else rows, stride))
        at += (rows - 1) * stride + row
    return layout


def test_lists_nv12_and_the_stream(S, cascade_paths, oracle):
    prm = S.Params(max_width=640, max_height=480, max_frames=4)
    f = S.ERFilter(params=prm)
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    sy, cr = S.synth, _crops()
    flags = GROUPED | S.WANT_LINE_CROPS | S.WANT_LINE_GLYPHS
    frames = [sy.stext_bgr(sy.frame_seed(2), 640, 480), cr[2], sy.stext_bgr(sy.frame_seed(831), 321, 243), sy.snoise_bgr(sy.frame_seed(832), 97, 61)]
    lst = f.text_detect_list(frames, flags)
    singles = [f.text_detect(fr, flags) for fr in frames]
    for i in range(len(frames)):
        assert _frame_crops(lst, i) == _frame_crops(singles[i], 0)
    assert len(lst.texts) > 0
    # NV12 list against one NV12 call per frame, and the grey crops against the luma the oracle converts
    nvf = [sy.stext_bgr(sy.frame_seed(2), 640, 480), sy.stext_bgr(sy.frame_seed(834), 322, 244)]
    nv = [sy.nv12_from_bgr(b) for b in nvf]
    nres = f.text_detect_nv12_list(nv, flags | S.WANT_MASKS)
    for i, (n, b) in enumerate(zip(nv, nvf)):
        assert _frame_crops(nres, i) == _frame_crops(f.text_detect_nv12(n, b.shape[1], b.shape[0], flags), 0)
    lumas = [oracle.nv12_to_ycrcb(n, b.shape[1], b.shape[0])[0] for n, b in zip(nv, nvf)]
    y_of = lambda fr, p: lumas[fr]                                  # noqa: E731
    check_crops(nres, y_of, union_of=mask_union(nres, y_of))
    # the stream, depth 3: a uniform batch, a BGR list and an NV12 list, byte-identical to the blocking calls
    same = np.stack([sy.stext_bgr(sy.frame_seed(s), 640, 480) for s in (2, 835)])
    uni = f.text_detect(same, flags)
    st = S.FrameStream(prm, depth=3)
    st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
    st.submit_copy(same, flags)
    slot, buf = st.acquire()
    st.submit_list(slot, _place(buf, frames), flags)
    slot, buf = st.acquire()
    st.submit_nv12_list(slot, _place(buf, nv, bpp=1, rows_of=lambda r: r // 3 * 2), flags | S.WANT_MASKS)
    for exp in (uni, lst, nres):
        _, got = st.next()
        assert got.texts.tobytes() == exp.texts.tobytes()
        assert got.line_crops.tobytes() == exp.line_crops.tobytes()
        assert got.line_crop_pixels.tobytes() == exp.line_crop_pixels.tobytes()
        assert got.line_glyph_pixels.tobytes() == exp.line_glyph_pixels.tobytes()
    st.close(); f.close()


_DEVICE_CHILD = r"""
import sys
import numpy as np
import torch                                    # (first: the HIP runtime PyTorch brings, as in smoke())
sys.path.insert(0, sys.argv[1])
import importlib
S = importlib.import_module("scene-text-recognition_amd")
f = S.ERFilter(params=S.Params(max_width=640, max_height=480, max_frames=2))
f.load_cascade(0, sys.argv[2]); f.load_cascade(1, sys.argv[3])
sy = S.synth
flags = 7 | 32 | 64 | S.WANT_LINE_CROPS | S.WANT_LINE_GLYPHS
frames = [sy.stext_bgr(sy.frame_seed(2), 640, 480), sy.stext_bgr(sy.frame_seed(841), 333, 211)]
host = f.text_detect_list(frames, flags)
dev = [torch.from_numpy(np.ascontiguousarray(fr)).cuda() for fr in frames]
torch.cuda.synchronize()
res = f.detect_bgr_list_device([(t.data_ptr(), fr.shape[1], fr.shape[0], 3 * fr.shape[1]) for t, fr in zip(dev, frames)], flags)
assert res.texts.tobytes() == host.texts.tobytes() and len(res.texts) > 0
assert res.line_crops.tobytes() == host.line_crops.tobytes()
assert res.line_crop_pixels.tobytes() == host.line_crop_pixels.tobytes()
assert res.line_glyph_pixels.tobytes() == host.line_glyph_pixels.tobytes()
print("device crops ok", len(res.texts))
"""


def test_device_frames(S, cascade_paths):
    out = subprocess.run([sys.executable, "-c", _DEVICE_CHILD, ROOT, cascade_paths[0], cascade_paths[1]], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "device crops ok" in out.stdout


@pytest.mark.parametrize("height,max_width,pad", [(16, 1024, 0.0), (48, 1024, 0.25), (32, 16, 0.125)])
def test_crop_settings(S, cascade_paths, oracle, height, max_width, pad):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=2)
    f.set_line_crop(height, max_width, pad)
    sy = S.synth
    frames = [sy.stext_bgr(sy.frame_seed(2), 640, 480), _crops()[0]]
    res = f.text_detect_list(frames, GROUPED, want_line_crops=True)
    ys = [oracle.compute_channels(fr)[0] for fr in frames]
    assert check_crops(res, lambda fr, p: ys[fr], height, max_width, pad) > 0
    assert (res.line_crops["height"] == height).all() and (res.line_crops["width"] <= max_width).all()
    if max_width == 16:
        assert (res.line_crops["width"] == 16).any()               # a line squeezed to max_width
    batch, widths = res.line_crop_batch()
    assert batch.shape == (len(res.texts), height, int(widths.max()))
    f.close()


# ---- str_er_line_crops on hand-made geometry: the kernel's own edges, placed exactly ------------------------------------------------------
# The detector's lines have slopes near 0, lie inside the frame and get heights that are multiples of 8.  str_er_line_crops takes any
# boxes, so these cases put the taps where the kernel can go wrong: clamped on each side of the plane, at negative source coordinates,
# along steep slopes, many source pixels apart, and in crops whose 4-byte quads wrap from one row to the next or end with 1 to 3 bytes.

HAND_PW, HAND_PH = 97, 61


def _taps(g, pw, ph):
    """Of the reference's taps of geometry g on a pw x ph plane: how many lie left of, right of, above and below the plane, and (sx, sy)."""
    sx, sy = REF._coords(g)
    x0, y0 = sx >> 16, sy >> 16
    return {"left": int((x0 < 0).sum()), "right": int((x0 + 1 > pw - 1).sum()), "above": int((y0 < 0).sum()), "below": int((y0 + 1 > ph - 1).sum()),
            "any": int(((x0 < 0) | (x0 + 1 > pw - 1) | (y0 < 0) | (y0 + 1 > ph - 1)).sum()), "n": int(x0.size)}, sx, sy


def _hand_cases():
    """[(name, (height, max_width, pad), [(boxes, slope), ...])]: the lines of one entry go through one call at its settings."""
    return [("top_left", (32, 1024, 0.25), [([(0, 0, 40, 14)], 0.3)]),
            ("bottom_right", (48, 1024, 0.25), [([(70, 47, 27, 14)], -0.4)]),
            ("whole_plane", (16, 1024, 0.125), [([(0, 0, HAND_PW, HAND_PH)], 3.0)]),
            ("outside_and_column", (32, 1024, 0.0), [([(-40, -20, 30, 10)], 0.0), ([(40, 10, 1, 40)], 0.0)]),
            ("squeezed", (32, 5, 0.125), [([(0, 25, HAND_PW, 6)], 0.01)]),
            ("tall_padded", (256, 8192, 1.0), [([(60, 40, 18, 19), (82, 42, 18, 15)], 0.0)]),
            ("height_9", (9, 1024, 0.0), [([(10, 10, w, 9)], 0.0) for w in (13, 14, 15)] + [([(3, 30, 21, 9)], 0.25)]),
            ("height_11", (11, 1024, 0.0), [([(20, 5, w, 11)], 0.0) for w in (5, 6, 7)] + [([(50, 40, 17, 11)], -0.3)])]


def _check_reaches(name, lines, settings):
    """What each case was made for, from the reference's own coordinates: a later change of the numbers cannot empty a case."""
    gs = [REF.geometry(b, s, *settings) for b, s in lines]
    t, sx, sy = _taps(gs[0], HAND_PW, HAND_PH)
    if name == "top_left":
        assert t["left"] > 0 and t["above"] > 0
        assert (((sx >> 8) & 255)[sx < 0] != 0).any() and (((sy >> 8) & 255)[sy < 0] != 0).any()       # negative coordinates with a fraction
    elif name == "bottom_right":
        assert t["right"] > 0 and t["below"] > 0 and gs[0][0] == 59 and gs[0][0] % 4 == 3
    elif name == "whole_plane":
        assert min(t["left"], t["right"], t["above"], t["below"]) > 0 and abs(gs[0][5]) > abs(gs[0][4])           # steep: uy beyond ux
    elif name == "outside_and_column":
        assert ((sx >> 16) + 1 <= 0).all() and ((sy >> 16) + 1 <= 0).all()                                       # every tap is pixel (0, 0)
        assert gs[1][0] == 1
    elif name == "squeezed":
        assert gs[0][0] == 5 and gs[0][4] >= 15 * 65536                                                           # many source pixels a column
    elif name == "tall_padded":
        assert gs[0][:2] == (351, 256) and 3 * t["any"] >= t["n"]
    else:
        assert {g[0] * g[1] % 4 for g in gs} == {1, 2, 3} and all(g[0] % 4 for g in gs)                           # a last quad of 1, 2 and 3 bytes


def _run_hand(f, plane, name, settings, lines):
    """All lines of a case in one call and one at a time: records, layout, padding, and every byte against the numpy sampler."""
    f.set_line_crop(*settings)
    boxes = np.array([b for bs, _ in lines for b in bs])
    count = [len(bs) for bs, _ in lines]
    first = np.concatenate([[0], np.cumsum(count)[:-1]])
    recs, pixels = f.line_crops(plane, boxes, first, count, [s for _, s in lines])
    assert len(recs) == len(lines)
    off, crops = 0, []
    for rec, (bs, s) in zip(recs, lines):
        exp = REF.geometry(bs, s, *settings)
        got = REF.fields(rec)
        assert got[:2] == exp[:2], name
        assert all(abs(a - b) <= 1 for a, b in zip(got[2:], exp[2:])), (name, got, exp)
        assert int(rec["pix_off"]) == off and off % 4 == 0
        nb = got[0] * got[1]
        crop = pixels[off:off + nb].reshape(got[1], got[0])
        assert (crop == REF.sample_grey(plane, got)).all(), (name, plane.shape, bs)
        off += (nb + 3) // 4 * 4
        assert not pixels[int(rec["pix_off"]) + nb:off].any(), name          # the padding between the crops
        crops.append(crop)
    assert off == len(pixels)
    for k, (bs, s) in enumerate(lines):
        r1, p1 = f.line_crops(plane, np.array(bs), [0], [len(bs)], [s])
        assert REF.fields(r1[0]) == REF.fields(recs[k]) and int(r1[0]["pix_off"]) == 0
        assert p1[:crops[k].size].tobytes() == crops[k].tobytes() and len(p1) == (crops[k].size + 3) // 4 * 4 and not p1[crops[k].size:].any()
    return crops


def test_line_crops_hand_made_geometry(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=1)
    rng = np.random.default_rng(61)
    noise = rng.integers(0, 256, (HAND_PH, HAND_PW), dtype=np.uint8)
    noise[0, 0], noise[HAND_PH - 1, HAND_PW - 1], noise[0, HAND_PW - 1], noise[HAND_PH - 1, 0] = 7, 255, 0, 200
    cases = _hand_cases()
    for name, settings, lines in cases:
        _check_reaches(name, lines, settings)
        crops = _run_hand(f, noise, name, settings, lines)
        if name == "outside_and_column":
            assert (crops[0] == 7).all()                                    # the corner pixel alone
    # planes one pixel wide or high: every tap is clamped along that axis
    for shape in ((HAND_PH, 1), (1, HAND_PW), (1, 1)):
        thin = rng.integers(0, 256, shape, dtype=np.uint8)
        for name, settings, lines in cases:
            _run_hand(f, thin, name, settings, lines)
    # interpolation between equal values, and the rounding, must not lose a level at the top
    white = np.full((HAND_PH, HAND_PW), 255, np.uint8)
    for name, settings, lines in cases:
        assert all((c == 255).all() for c in _run_hand(f, white, name, settings, lines)), name
    f.set_line_crop()
    f.close()


def test_errors(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=1)
    frame = S.synth.stext_bgr(S.synth.frame_seed(2), 640, 480)
    good = f.text_detect(frame, GROUPED, want_line_crops="glyphs")
    assert len(good.texts) > 0

    def still_ok():
        again = f.text_detect(frame, GROUPED, want_line_crops="glyphs")
        assert again.line_crop_pixels.tobytes() == good.line_crop_pixels.tobytes()
        assert again.line_glyph_pixels.tobytes() == good.line_glyph_pixels.tobytes()

    for stages in (7 | 32 | S.WANT_LINE_CROPS, 7 | 32 | S.WANT_LINE_CROPS | S.WANT_LINE_GLYPHS, 7 | S.WANT_LINE_GLYPHS, GROUPED | S.WANT_LINE_GLYPHS):
        with pytest.raises(S.StrErError) as e:
            f.text_detect(frame, stages)
        assert e.value.code == -1, stages
        still_ok()
    import ctypes as C
    blob = (C.c_char * 16)()
    blobs = (C.c_void_p * 1)(C.cast(blob, C.c_void_p))
    sizes = (C.c_int64 * 1)(16)
    for flag in (S.WANT_LINE_CROPS, S.WANT_LINE_CROPS | S.WANT_LINE_GLYPHS):
        rh = C.c_void_p()
        rc = f.L.str_er_strip_merge(f.h, frame.ctypes.data, 640, 480, 1920, 0, C.cast(blobs, C.c_void_p), C.cast(sizes, C.c_void_p), 1,
                                    GROUPED | flag, C.byref(rh))
        assert rc == -1 and b"WANT_LINE_CROPS" in f.L.str_er_last_error(f.h)
        still_ok()
    for bad in ((7, 1024, 0.1), (257, 1024, 0.1), (32, 0, 0.1), (32, 8193, 0.1), (32, 64, -0.5), (32, 64, 1.01), (32, 64, float("nan"))):
        with pytest.raises(S.StrErError) as e:
            f.set_line_crop(*bad)
        assert e.value.code == -1
        still_ok()                                                  # the settings are unchanged
    y = f.compute_channels(frame)[0]
    with pytest.raises(S.StrErError):
        f.line_crops(y, np.array([[0, 0, 0, 5]]), [0], [1], [0.0])
    still_ok()
    f.close()


def test_single_stage_equals_fused(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=1)
    frame = S.synth.stext_bgr(S.synth.frame_seed(2), 640, 480)
    f.set_line_crop(40, 512, 0.2)
    res = f.text_detect(frame, GROUPED, want_line_crops=True)
    n = len(res.texts)
    assert n > 0
    boxes, first, count = [], [], []
    for t in range(n):
        b, _ = _boxes(res, t)
        first.append(len(boxes)); count.append(len(b))
        boxes.extend(b.tolist())
    recs, pixels = f.line_crops(f.compute_channels(frame)[0], np.array(boxes), first, count, res.texts["slope"])
    assert recs.tobytes() == res.line_crops.tobytes()
    assert pixels.tobytes() == res.line_crop_pixels.tobytes()
    # sizing: without pixels only the records and the byte count; a cap one byte short is ECAPACITY with the count set
    import ctypes as C
    y = np.ascontiguousarray(f.compute_channels(frame)[0])
    bx, fi, co, sl = (np.ascontiguousarray(np.array(boxes), np.int32), np.asarray(first, np.int32), np.asarray(count, np.int32),
                      np.ascontiguousarray(res.texts["slope"], np.float64))
    r2 = np.zeros(n, S.LINE_CROP_DTYPE)
    nb = C.c_uint64()
    short = np.zeros(len(pixels) - 1, np.uint8)
    rc = f.L.str_er_line_crops(f.h, y.ctypes.data, 640, 480, 640, bx.ctypes.data, fi.ctypes.data, co.ctypes.data, sl.ctypes.data, n,
                               short.ctypes.data, len(short), C.byref(nb), r2.ctypes.data)
    assert rc == -7 and nb.value == len(pixels) and r2.tobytes() == recs.tobytes()
    f.close()


def test_cpp_example(S, cascade_paths, tmp_path):
    libdir = os.path.dirname(S.lib_path())
    exe = str(tmp_path / "example_line_crops")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "scene-text-recognition_amd", "host", "example_line_crops.cpp"),
                    "-I", os.path.join(ROOT, "include"), "-L", libdir, "-lstr_er_hip", f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    frame = S.synth.stext_bgr(S.synth.frame_seed(2), 640, 480)
    raw = tmp_path / "f.bgr"
    raw.write_bytes(np.ascontiguousarray(frame).tobytes())
    out_dir = tmp_path / "crops"
    out_dir.mkdir()
    out = subprocess.run([exe, cascade_paths[0], cascade_paths[1], str(raw), "640", "480", str(out_dir)], check=True, capture_output=True,
                         text=True).stdout.splitlines()
    assert out[-1].endswith("fused == single-stage: yes")
    f = S.ERFilter(params=S.Params(thresh_step=8, min_area=120, max_area=900000, max_width=640, max_height=480))
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    res = f.text_detect(frame, GROUPED, want_line_crops="glyphs")
    lines = [l.split() for l in out if l.startswith("line ")]
    assert len(lines) == len(res.texts) > 0
    for t, l in enumerate(lines):
        crop = res.line_crop(t)
        assert [int(v) for v in l[1:]] == [t, crop.shape[1], crop.shape[0], int(crop.astype(np.int64).sum())]
        pgm = (out_dir / f"line_{t}.pgm").read_bytes()
        assert pgm.endswith(crop.tobytes()) and pgm.startswith(f"P5\n{crop.shape[1]} {crop.shape[0]}\n255\n".encode())
        assert (out_dir / f"glyph_{t}.pgm").read_bytes().endswith(res.line_glyph(t).tobytes())
    f.close()
