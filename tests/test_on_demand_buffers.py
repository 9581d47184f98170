"""The on-demand buffers of a context (masks, crops, maps, footprints, link and geometry tables) grow and are reused: one context
runs the single-stage calls on a small plane, on a large one and on the small one again.  Every output is compared with the reference
its own test module uses, the third round equals the first byte for byte, and none of it shows in workspace_bytes().
The buffers behind feet_geom -- those of the reading chain, feet_words to decode_tracks and the track pools -- are test_read_chain_reuse.py's."""
import numpy as np
import pytest

import frame_lines_ref as FR
import line_geom_ref as GR
import line_links_ref as LR
from shape_ref import as_dict, shape_ref
from test_er_masks import flood, pack
from test_line_crops import REF as CR
from text_map_ref import Raster

pytestmark = pytest.mark.gpu


def _scene(rng, pw, ph, rects):
    """A bright plane with dark rectangles (x, y, w, h), a few bright pixels inside each: one region per rectangle, its key the corner."""
    plane = (rng.random((ph, pw)) * 40 + 200).astype(np.uint8)
    boxes = []
    for x, y, w, h in rects:
        plane[y:y + h, x:x + w] = 0
        holes = rng.random((h, w)) < 0.03
        holes[0, 0] = False
        plane[y:y + h, x:x + w][holes] = 247
        boxes.append((x, y, w, h, y * pw + x, 0))
    return plane, boxes


def _small(rng):
    return _scene(rng, 64, 48, [(9, 7, 40, 30)])


def _large(rng):
    """90 rectangles on a grid of 64 x 40 cells, and one of 620 x 110: its rows take more than the mask kernels' LDS (global scratch)."""
    rects = []
    for r in range(9):
        for c in range(10):
            w, h = int(rng.integers(20, 57)), int(rng.integers(10, 35))
            rects.append((64 * c + int(rng.integers(1, 63 - w)), 40 * r + int(rng.integers(1, 39 - h)), w, h))
    rects.append((10, 364, 620, 110))
    assert 110 * ((620 + 63) // 64) > 1024
    return _scene(rng, 640, 480, rects)


def _lines(n):
    """Two regions to a line, and a last line of the first four regions again (it shares pixels with lines 0 and 1)."""
    line_of = [k // 2 for k in range(n)]
    n_lines = (n + 1) // 2 + 1
    again = list(range(min(4, n)))
    return list(range(n)) + again, line_of + [n_lines - 1] * len(again), n_lines


def _run(S, f, plane, boxes):
    """Every single-stage call on the regions of one plane; the outputs by name."""
    ph, pw = plane.shape
    n = len(boxes)
    regs = np.zeros(n, S.CAND_DTYPE)
    for i, (x, y, w, h, key, level) in enumerate(boxes):
        regs[i]["x"], regs[i]["y"], regs[i]["w"], regs[i]["h"], regs[i]["key"], regs[i]["level"] = x, y, w, h, key, level
    out = {}
    out["mask_words"], out["mask_pixels"] = f.er_masks(plane, regs)
    out["shapes"] = f.er_shapes(plane, regs)
    xywh = np.array([b[:4] for b in boxes], np.int32)
    out["crops"], out["crop_pixels"] = f.line_crops(plane, xywh, list(range(n)), [1] * n, [0.0] * n)
    out["map"], out["ids"] = f.text_map_regions(plane, regs, [1 + k % 7 for k in range(n)], pw, ph, ids=list(range(n)))
    who, line_of, n_lines = _lines(n)
    out["feet"], out["foot_bits"], out["pairs"] = f.line_feet_regions(plane, regs[who], line_of, n_lines, pw, ph)
    out["links"] = f.link_feet(pw, ph, out["feet"], out["foot_bits"], out["feet"], out["foot_bits"])
    out["geoms"], out["points"] = f.feet_geom(pw, ph, out["feet"], out["foot_bits"])
    return out


def _check(oracle, plane, boxes, out):
    ph, pw = plane.shape
    n = len(boxes)
    q = oracle.quant_lut(8)[plane]
    masks = [flood(q, *b) for b in boxes]
    assert not all(m.all() for m in masks)
    assert (out["mask_words"] == np.concatenate([pack(m) for m in masks])).all()
    assert [int(p) for p in out["mask_pixels"]] == [int(m.sum()) for m in masks]
    for i, (x, y, w, h, _, _) in enumerate(boxes):
        assert as_dict(out["shapes"][i]) == shape_ref(masks[i], plane[y:y + h, x:x + w]), i
    off = 0
    for i, rec in enumerate(out["crops"]):
        exp, got = CR.geometry(np.array([boxes[i][:4]], np.int64), 0.0), CR.fields(rec)
        assert got[:2] == exp[:2] and all(abs(a - b) <= 1 for a, b in zip(got[2:], exp[2:])), i
        assert int(rec["pix_off"]) == off
        size = got[0] * got[1]
        assert (out["crop_pixels"][off:off + size].reshape(got[1], got[0]) == CR.sample_grey(plane, got)).all(), i
        off += (size + 3) // 4 * 4
    assert off == len(out["crop_pixels"])
    R = Raster(pw, ph)
    for i, (x, y, *_r) in enumerate(boxes):
        R.add(pw, ph, x, y, masks[i], 1 + i % 7, i)
    assert (out["map"] == R.map).all() and (out["ids"] == R.id_map()).all()
    who, line_of, n_lines = _lines(n)
    mem = [[] for _ in range(n_lines)]
    for k, t in zip(who, line_of):
        mem[t].append((pw, ph, boxes[k][0], boxes[k][1], masks[k]))
    feet = [FR.footprint(pw, ph, m) for m in mem]
    assert [tuple(int(g[k]) for k in ("x", "y", "w", "h", "pixels")) for g in out["feet"]] == [(r.x, r.y, r.w, r.h, r.pixels) for r in feet]
    assert (out["foot_bits"] == np.concatenate([r.words() for r in feet])).all()
    pairs = FR.all_pairs(feet, [0] * n_lines)
    assert [(int(p["a"]), int(p["b"]), int(p["inter"])) for p in out["pairs"]] == pairs and len(pairs) >= 1
    dup, frame_line, _, _ = FR.frame_lines([(r.x, r.y, r.w, r.h) for r in feet], [r.pixels for r in feet], [0] * n_lines, [0] * n_lines, pairs)
    assert [int(p["dup"]) for p in out["pairs"]] == dup and [int(g["frame_line"]) for g in out["feet"]] == frame_line
    assert [(int(p["a"]), int(p["b"]), int(p["inter"]), int(p["link"])) for p in out["links"]] == LR.set_links(feet, feet)
    assert len(out["geoms"]) == n_lines
    for t, r in enumerate(feet):
        msg = GR.same(out["geoms"][t], out["points"], GR.geom(r.bits, r.x, r.y))
        assert msg is None, (t, msg)


def test_buffers_grow_and_are_reused(S, cascade_paths, oracle):
    f = S.ERFilter(params=S.Params(max_width=640, max_height=480, max_frames=1))
    f.load_cascade(0, cascade_paths[0])
    f.load_cascade(1, cascade_paths[1])
    ws = f.workspace_bytes()
    small, large = _small(np.random.default_rng(21)), _large(np.random.default_rng(22))
    first = _run(S, f, *small)
    _check(oracle, *small, first)
    big = _run(S, f, *large)
    _check(oracle, *large, big)
    assert len(big["mask_words"]) > 16 * len(first["mask_words"]) and len(big["foot_bits"]) > 16 * len(first["foot_bits"])
    third = _run(S, f, *small)
    assert sorted(third) == sorted(first)
    for k in first:
        assert third[k].tobytes() == first[k].tobytes(), k
    assert f.workspace_bytes() == ws
    f.close()
