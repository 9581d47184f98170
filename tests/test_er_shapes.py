"""Region descriptors (STR_ER_WANT_SHAPES, str_er_er_shapes) on the GPU: every record against the numpy / scipy reference of the
contract on the candidate's mask and plane, nothing else of a call changed by the flag, lists / NV12 / the stream / device frames,
hand-made shapes for every size class of the kernels and for boxes wider than 4096 pixels, the single-stage call against the fused one,
and the errors."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import ndimage

from box_round_cases import mask_class
from shape_ref import FOUR, as_dict, shape_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _crops():
    z = np.load(os.path.join(GOLDEN, "icdar_crops.npz"))
    return [np.ascontiguousarray(z[k]) for k in sorted(z.files)]


def _ctx(S, cascade_paths, **kw):
    f = S.ERFilter(params=S.Params(**kw))
    f.load_cascade(0, cascade_paths[0])
    f.load_cascade(1, cascade_paths[1])
    return f


def check_shapes(oracle, res, plane_of):
    """Every candidate: record == shape_ref(mask, P' under the box); pixels == the oracle node's npix."""
    assert res.shapes is not None and len(res.shapes) == len(res.cands)
    n = 0
    for p_i, p in enumerate(res.planes):
        if not len(p.cands):
            continue
        img = plane_of(p)
        npix = {(int(t["key"]), int(t["level"])): int(t["npix"]) for t in oracle.tree_extract(img, step=8).nodes}
        first = int(np.nonzero(res.cands["plane"] == p_i)[0][0])
        for k, c in enumerate(p.cands):
            i = first + k
            x, y, w, h = int(c["x"]), int(c["y"]), int(c["w"]), int(c["h"])
            assert as_dict(res.shapes[i]) == shape_ref(res.mask(i), img[y:y + h, x:x + w]), (p_i, i)
            assert int(res.shapes[i]["pixels"]) == npix[(int(c["key"]), int(c["level"]))]
            n += 1
    return n


def test_fused_shapes_match_the_reference(S, cascade_paths, oracle):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=8)
    sy = S.synth
    frames = _crops() + [sy.stext_bgr(sy.frame_seed(900), 640, 480), sy.snoise_bgr(sy.frame_seed(901), 200, 100)]
    res = f.text_detect_list(frames, want_masks=True, want_shapes=True)
    six = [oracle.compute_channels(fr) for fr in frames]
    n = check_shapes(oracle, res, lambda p: six[p.frame][p.ch])
    assert n == len(res.cands) > 20
    assert (res.shapes["euler"] < 1).any() and (res.shapes["hole_pixels"] > 0).any()      # the data has holes
    f.close()


def test_fused_shapes_pyramid_1080p(S, cascade_paths, oracle):
    L = 8
    f = _ctx(S, cascade_paths, max_width=1920, max_height=1080, max_frames=1, n_pyr_levels=L, channel_mask=0x07)
    frame = S.synth.stext_bgr(S.synth.frame_seed(910), 1920, 1080)
    res = f.text_detect(frame, want_masks=True, want_shapes=True)
    six = oracle.compute_channels(frame)
    pyr = {c: oracle.pyramid(six[c], L) for c in range(3)}
    assert {p.pyr for p in res.planes} == set(range(L))
    n = check_shapes(oracle, res, lambda p: pyr[p.ch][p.pyr])
    assert n == len(res.cands) > 20
    alone = f.text_detect(frame, want_shapes=True)
    assert alone.masks is None and alone.shapes.tobytes() == res.shapes.tobytes()
    f.close()


FIELDS = ("info", "cands", "tracks", "texts", "text_ers", "group_bounds", "group_all", "ocr_label", "ocr_prob", "line_crops",
          "line_crop_pixels", "line_glyph_pixels")


def _same(a, b):
    for k in FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), k
        if x is not None:
            assert x.tobytes() == y.tobytes(), k
    for pa, pb in zip(a.planes, b.planes):
        assert (pa.nodes is None) == (pb.nodes is None)
        if pa.nodes is not None:
            assert pa.nodes.tobytes() == pb.nodes.tobytes()


def test_shapes_change_nothing_else(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=4)
    sy = S.synth
    frames = [sy.stext_bgr(sy.frame_seed(2), 640, 480), _crops()[1], sy.snoise_bgr(sy.frame_seed(921), 200, 100)]
    stages = S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP | S.WANT_NODES | S.WANT_LINE_CROPS | S.WANT_LINE_GLYPHS
    plain = f.text_detect_list(frames, stages)
    shaped = f.text_detect_list(frames, stages | S.WANT_SHAPES)
    masked = f.text_detect_list(frames, stages | S.WANT_MASKS)
    both = f.text_detect_list(frames, stages | S.WANT_MASKS | S.WANT_SHAPES)
    again = f.text_detect_list(frames, stages)
    assert plain.shapes is None and masked.shapes is None and again.shapes is None
    assert shaped.masks is None and shaped.shapes is not None
    for r in (shaped, masked, both, again):
        _same(plain, r)
    assert both.masks.tobytes() == masked.masks.tobytes() and both.mask_bits.tobytes() == masked.mask_bits.tobytes()
    assert shaped.shapes.tobytes() == both.shapes.tobytes()
    assert plain.texts is not None and len(plain.texts) > 0 and len(plain.cands) > 20
    f.close()


def _frame_shapes(res, i):
    return res.shapes[res.cands["frame"] == i]


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
    frames = [sy.stext_bgr(sy.frame_seed(930), 640, 480), cr[2], sy.stext_bgr(sy.frame_seed(931), 321, 243), sy.snoise_bgr(sy.frame_seed(932), 97, 61)]
    lst = f.text_detect_list(frames, want_shapes=True)
    for i, fr in enumerate(frames):
        assert _frame_shapes(lst, i).tobytes() == f.text_detect(fr, want_shapes=True).shapes.tobytes()
    nvf = [sy.stext_bgr(sy.frame_seed(933), 640, 480), sy.stext_bgr(sy.frame_seed(934), 322, 244)]
    nv = [sy.nv12_from_bgr(b) for b in nvf]
    nres = f.text_detect_nv12_list(nv, S.STAGE_ALL | S.WANT_SHAPES | S.WANT_MASKS)
    three = [oracle.nv12_to_ycrcb(n, b.shape[1], b.shape[0]) for n, b in zip(nv, nvf)]
    assert check_shapes(oracle, nres, lambda p: 255 - three[p.frame][p.ch % 3] if p.ch >= 3 else three[p.frame][p.ch]) > 0
    for i, n in enumerate(nv):
        one = f.text_detect_nv12(n, nvf[i].shape[1], nvf[i].shape[0], S.STAGE_ALL | S.WANT_SHAPES)
        assert _frame_shapes(nres, i).tobytes() == one.shapes.tobytes()
    st = S.FrameStream(prm, depth=3)
    st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
    slot, buf = st.acquire()
    st.submit_list(slot, _place(buf, frames), S.STAGE_ALL | S.WANT_SHAPES)
    slot, buf = st.acquire()
    st.submit_nv12_list(slot, _place(buf, nv, bpp=1, rows_of=lambda r: r // 3 * 2), S.STAGE_ALL | S.WANT_SHAPES)
    _, a = st.next()
    _, b = st.next()
    for got, exp in ((a, lst), (b, nres)):
        assert got.cands.tobytes() == exp.cands.tobytes() and got.masks is None
        assert got.shapes.tobytes() == exp.shapes.tobytes()
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
frames = [sy.stext_bgr(sy.frame_seed(940), 640, 480), sy.stext_bgr(sy.frame_seed(941), 333, 211)]
host = f.text_detect_list(frames, want_shapes=True)
dev = [torch.from_numpy(np.ascontiguousarray(fr)).cuda() for fr in frames]
torch.cuda.synchronize()
res = f.detect_bgr_list_device([(t.data_ptr(), fr.shape[1], fr.shape[0], 3 * fr.shape[1]) for t, fr in zip(dev, frames)], S.STAGE_ALL | S.WANT_SHAPES)
assert res.cands.tobytes() == host.cands.tobytes() and res.shapes.tobytes() == host.shapes.tobytes()
assert len(res.cands) > 0
print("device shapes ok", len(res.cands))
"""


def test_device_frames(S, cascade_paths):
    out = subprocess.run([sys.executable, "-c", _DEVICE_CHILD, ROOT, cascade_paths[0], cascade_paths[1]], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "device shapes ok" in out.stdout


# ---- str_er_er_shapes on hand-made planes --------------------------------------------------------------------------------------------

def _regions(S, boxes):
    r = np.zeros(len(boxes), S.CAND_DTYPE)
    for i, (x, y, w, h, key, level) in enumerate(boxes):
        r[i]["x"], r[i]["y"], r[i]["w"], r[i]["h"], r[i]["key"], r[i]["level"] = x, y, w, h, key, level
    return r


def _expect(q, plane, x, y, w, h, key, level):
    ky, kx = divmod(int(key), q.shape[1])
    lab, _ = ndimage.label(q[y:y + h, x:x + w] <= level, structure=FOUR)
    return shape_ref(lab == lab[ky - y, kx - x], plane[y:y + h, x:x + w])


def _spiral(W, H):
    """A 1-pixel corridor (0) spiralling inwards between 1-pixel walls (255): its walls are one long spiral too, the worst case of
    the hole flood (every sweep advances it by about one turn)."""
    p = np.full((H, W), 255, np.uint8)
    t, b, l, r = 0, H - 1, 0, W - 1
    p[t, l:r + 1] = 0
    while True:
        if b - t < 2:
            break
        p[t:b + 1, r] = 0
        if r - l < 2:
            break
        p[b, l:r + 1] = 0
        t += 2
        if b - t < 2:
            break
        p[t:b + 1, l] = 0
        r -= 2
        if r - l < 2:
            break
        p[t, l:r + 1] = 0
        b -= 2
        l += 2
    return p


def _rings(n):
    """Concentric square corridors (0) two pixels apart, each joined to the next inner one by one gap: the walls between them are
    nested holes."""
    p = np.full((n, n), 255, np.uint8)
    d = 0
    while n - 2 * d >= 3:
        p[d, d:n - d] = p[n - 1 - d, d:n - d] = 0
        p[d:n - d, d] = p[d:n - d, n - 1 - d] = 0
        d += 2
    for k, dd in enumerate(range(1, d - 1, 2)):
        p[dd if k % 2 == 0 else n - 1 - dd, n // 2] = 0
    return p


def _diagonals():
    """Small rings (0) on 255: two hole pixels that touch diagonally, a ring whose gap is only diagonal, a ring with a grey island."""
    p = np.full((20, 40), 255, np.uint8)
    p[1:5, 1:5] = 0; p[2, 2] = p[3, 3] = 255                   # one hole of two pixels
    p[1:4, 10:13] = 0; p[1, 12] = p[2, 11] = 255                # the hole pixel leaks through the corner
    p[1:8, 20:27] = 0; p[2:7, 21:26] = 255; p[4, 23] = 100      # a ring, an island the flood at level 0 does not reach
    return p


@pytest.mark.parametrize("step", [8, 13])
def test_er_shapes_hand_made(S, cascade_paths, oracle, step):
    f = _ctx(S, cascade_paths, max_width=1920, max_height=1080, max_frames=1, thresh_step=step)
    lut = oracle.quant_lut(step)
    cases = []
    sp = _spiral(200, 1000)                                     # scratch class: 1000 rows of 4 words
    cases.append((sp, [(0, 0, 200, 1000, 0, 0)]))
    for n in (200, 61):                                         # LDS class, small class
        cases.append((_rings(n), [(0, 0, n, n, 0, 0)]))
    yy, xx = np.mgrid[0:70, 0:130]
    cb = np.where((xx + yy) % 2 == 0, 0, 255).astype(np.uint8)
    cases.append((cb, [(0, 0, 64, 64, 0, 0), (0, 0, 130, 70, 0, 0)]))
    cases.append((np.zeros((1, 16384), np.uint8), [(0, 0, 16384, 1, 0, 0), (100, 0, 1, 1, 100, 0)]))
    cases.append((np.zeros((1080, 3), np.uint8), [(1, 0, 1, 1080, 1, 0), (0, 0, 3, 1080, 2, 0)]))
    dg = _diagonals()
    cases.append((dg, [(1, 1, 4, 4, 1 * 40 + 1, 0), (10, 1, 3, 3, 1 * 40 + 10, 0), (20, 1, 7, 7, 1 * 40 + 20, 0),
                       (20, 1, 7, 7, 1 * 40 + 20, int(lut[100]))]))
    yy, xx = np.mgrid[0:300, 0:333]
    grad = ((xx * 7 + yy * 3) % 256).astype(np.uint8)           # grey values under a large, ragged region
    cases.append((grad, [(0, 0, 333, 300, 0, int(lut[128])), (5, 5, 64, 40, 5 * 333 + 5, int(lut[200]))]))
    for plane, boxes in cases:
        q = lut[plane]
        got = f.er_shapes(plane, _regions(S, boxes))
        assert len(got) == len(boxes)
        for rec, b in zip(got, boxes):
            assert as_dict(rec) == _expect(q, plane, *b), (plane.shape, b)
    ring = as_dict(f.er_shapes(dg, _regions(S, [(20, 1, 7, 7, 1 * 40 + 20, 0)]))[0])
    assert ring["euler"] == 0 and ring["hole_pixels"] == 25                  # the island is hole
    assert as_dict(f.er_shapes(dg, _regions(S, [(1, 1, 4, 4, 41, 0)]))[0])["euler"] == 0
    assert as_dict(f.er_shapes(dg, _regions(S, [(10, 1, 3, 3, 50, 0)]))[0])["hole_pixels"] == 0
    f.close()


# ---- boxes wider than 4096 pixels: a lane owns 2 .. 4 words of a row, and neighbour bits cross from lane 63 to lane 0 of the next set ----

# (w, h): each words-per-lane count on both sides of the LDS / scratch line (h * ceil(w / 64) <= 1024 is the LDS class)
WIDE = ((4097, 15), (4097, 16), (4160, 15), (8193, 7), (8193, 8), (12289, 5), (12289, 6), (16384, 4), (16384, 5))


def _border_holes(W, H):
    """Level 0 everywhere but for wall pixels astride every word border x = 64 j, in three forms in turn: a 2 x 1 hole on the columns
    64 j - 1 and 64 j; two hole pixels that touch only diagonally across the border (one 8-connected hole); a pixel at 64 j - 1 whose
    only way out is the diagonal through a wall pixel of row 0 at column 64 j (a leak, not a hole)."""
    p = np.zeros((H, W), np.uint8)
    for j in range(1, (W - 1) // 64 + 1):
        x = 64 * j
        if j % 3 == 1:
            p[1, x - 1] = p[1, x] = 255
        elif j % 3 == 2:
            p[1, x - 1] = p[2, x] = 255
        else:
            p[1, x - 1] = p[0, x] = 255
    return p, 0, 0, 0


def _ragged(W, H, level_of):
    """A grey ramp under a ragged region, 255 elsewhere.  The rows h / 6, 3 h / 6 and 5 h / 6 (the crossing rows) start near column 0, so
    their runs cross every word border; the others start past column 4096 -- in the lane's second, third or fourth word of the row, a
    few columns further each row -- so their extents, and the hull's left side, come from those words alone.  Where the last word
    set has room the right ends are ragged as well.  The level is the highest there is: the ramp's values above 251 are pinholes
    (the crossing rows, one pixel high for most of their length, are capped at 251: a pinhole would cut them)."""
    wpl = ((W + 63) // 64 + 63) // 64
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = ((7 * xx + 3 * yy) % 256).astype(np.uint8)
    p = np.full((H, W), 255, np.uint8)
    room = W - 3 > 4096 * (wpl - 1) + 3 * H + 1
    for y in range(H):
        crossing = y in (H // 6, 3 * H // 6, 5 * H // 6)
        xl = 2 + y if crossing else min(4096 * (1 + y % max(1, wpl - 1)) + 3 * y + 1, W - 1)
        xr = W - y % 3 if room else W
        p[y, xl:xr] = np.minimum(ramp[y, xl:xr], 251) if crossing else ramp[y, xl:xr]
    level = int(level_of[251])
    ky = H // 6
    kx = int(np.nonzero(level_of[p[ky]] <= level)[0][0])
    return p, kx, ky, level


def test_er_shapes_wider_than_4096(S, cascade_paths, oracle):
    step = 8
    f = _ctx(S, cascade_paths, max_width=16384, max_height=600, max_frames=1, thresh_step=step)
    lut = oracle.quant_lut(step)
    assert int(lut[251]) == 255 // step < int(lut[252])
    assert [mask_class(w, h) for w, h in WIDE] == [1, 2, 1, 1, 2, 1, 2, 1, 2] and 4 * 256 == 1024
    assert [((w + 63) // 64 + 63) // 64 for w, h in WIDE] == [2, 2, 2, 3, 3, 4, 4, 4, 4]
    SW = 16384
    stack = np.full((2 * sum(h for _, h in WIDE), SW), 255, np.uint8)       # every plane below, one under the other, for the mixed call
    boxes, exps, y0 = [], [], 0
    for kind in ("holes", "ragged"):
        for w, h in WIDE:
            p, kx, ky, level = _border_holes(w, h) if kind == "holes" else _ragged(w, h, lut)
            exp = _expect(lut[p], p, 0, 0, w, h, ky * w + kx, level)
            if kind == "holes":                 # a hole and a leak on every word border, the borders between the lanes' word sets among them
                assert exp["hole_pixels"] > 0 and exp["euler"] < 0 and exp["crossings"][0] > 2, (w, h, exp)
                if (w, h) in ((4097, 15), (16384, 4)):
                    assert (exp["hole_pixels"], exp["euler"]) == {4097: (84, -41), 16384: (340, -169)}[w]
            else:                               # one region: every allowed pixel; rows that start past column 4096; runs on the crossing rows
                assert exp["pixels"] == int((lut[p] <= level).sum()) and min(exp["crossings"]) >= 2
                starts = [int(np.nonzero(row != 255)[0][0]) for row in p]
                assert max(starts) >= 4096 and min(starts) < 64 and exp["grey_sum2"] > exp["grey_sum"] > 0
            got = f.er_shapes(p, _regions(S, [(0, 0, w, h, ky * w + kx, level)]))
            assert as_dict(got[0]) == exp, (kind, w, h)
            stack[y0:y0 + h, :w] = p
            boxes.append((0, y0, w, h, (y0 + ky) * SW + kx, level))
            exps.append(exp)
            y0 += h
    # all of them in one call, and two boxes of the small class between them: the classes and the slots mixed
    q = lut[stack]
    for x, y, w, h in ((0, 0, 64, 15), (4090, 31, 64, 15)):
        boxes.append((x, y, w, h, y * SW + x, 0))
        exps.append(_expect(q, stack, *boxes[-1]))
    order = list(range(len(boxes) - 1, -1, -1))
    order.insert(5, order.pop()); order.insert(11, order.pop(0))
    assert sorted(order) == list(range(len(boxes))) and {mask_class(b[2], b[3]) for b in boxes} == {0, 1, 2}
    got = f.er_shapes(stack, _regions(S, [boxes[i] for i in order]))
    assert len(got) == len(order)
    for rec, i in zip(got, order):
        assert as_dict(rec) == exps[i], boxes[i]
    f.close()


def test_single_stage_equals_fused(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=1)
    frame = S.synth.stext_bgr(S.synth.frame_seed(950), 640, 480)
    res = f.text_detect(frame, want_shapes=True)
    planes = f.compute_channels(frame)
    n = 0
    for p_i, p in enumerate(res.planes):
        sel = np.nonzero(res.cands["plane"] == p_i)[0]
        if len(sel):
            assert f.er_shapes(planes[p.ch], res.cands[sel]).tobytes() == res.shapes[sel].tobytes()
            n += len(sel)
    assert n == len(res.cands) > 20
    f.close()


def test_errors(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=320, max_height=240, max_frames=1)
    frame = S.synth.stext_bgr(S.synth.frame_seed(960), 320, 240)
    blob = (C.c_char * 16)()
    blobs = (C.c_void_p * 1)(C.cast(blob, C.c_void_p))
    sizes = (C.c_int64 * 1)(16)
    rh = C.c_void_p()
    rc = f.L.str_er_strip_merge(f.h, frame.ctypes.data, 320, 240, 960, 0, C.cast(blobs, C.c_void_p), C.cast(sizes, C.c_void_p), 1,
                                S.STAGE_ALL | S.WANT_SHAPES, C.byref(rh))
    assert rc == -1 and b"WANT_SHAPES" in f.L.str_er_last_error(f.h)
    wide = np.zeros((1, 16385), np.uint8)
    with pytest.raises(S.StrErError) as e:
        f.er_shapes(wide, _regions(S, [(0, 0, 16385, 1, 0, 0)]))
    assert e.value.code == -7
    plane = np.zeros((100, 120), np.uint8)
    plane[50:, :] = 200
    good = _regions(S, [(0, 0, 120, 50, 0, 0), (3, 4, 33, 10, 4 * 120 + 3, 0)])
    hi = 255 // 8 + 1
    bad = {"box outside": (100, 0, 21, 5, 100, 0), "key outside": (0, 0, 10, 10, 20, 0), "key level": (0, 50, 10, 10, 50 * 120, 3),
           "sentinel": (0, 0, 10, 10, 0, hi)}
    for name, b in bad.items():
        with pytest.raises(S.StrErError) as e:
            f.er_shapes(plane, np.concatenate([good, _regions(S, [b])]))
        assert e.value.code == -1 and "region 2" in str(e.value), name
        assert list(f.er_shapes(plane, good)["pixels"]) == [120 * 50, 33 * 10]       # the context stays usable
    assert len(f.er_shapes(plane, good[:0])) == 0
    assert len(f.text_detect(frame, want_shapes=True).shapes) > 0
    f.close()
