"""The feature half of the OCR scorer at the kernels' own edges (ocr_kernels.hip: k_ocr_features, RotSrc / make_rot_geom, k_ocr_list,
k_ocr_list_from).

Every input (tests/ocr_cases.py) is made up for one property: ARAN(30)'s target size where 30 sqrt(w / h) is an integer -- or, in five
shapes, truncates below it --, the copy and exact-2x resize forms, constant / three-level / ramp ROIs that put the Otsu threshold on
show in q, marks on the tile's border, rotate_mat's uncropped fall-back, negative crop heights and one-pixel canvases, box counts around
the four boxes of a workgroup and the 64 of a k_ocr_otsu block, candidate totals around the lister's 4096-candidate chunk.  The CPU
section proves on the oracle and on plain restatements of the constants and the geometry that each input has the property it was made
for; the GPU section compares chain_run's q rows with the oracle's chain_features (np.array_equal) and the fused STAGE_OCR with chain_run
on the same box (==).  Nothing is skipped or filtered and there is no tolerance.

The ARAN boxes lie on a 960 x 960 plane: the listed shapes 1 x 901 and 1 x 960 do not fit a 900 x 900 one.
"""
import gzip
import math

import numpy as np
import pytest

import cascade_cases as cc
import ocr_cases as oc


@pytest.fixture(scope="module")
def refs(oracle):
    return oc.Refs(oracle)


def _aran(refs):
    plane = refs.plane("aran", oc.aran_plane)
    return plane, oc.aran_boxes()


def _forms(refs):
    return refs.plane("forms", oc.form_plane)


def _slant(refs):
    return refs.plane("slant", oc.slant_plane)


def _pow_root(r):
    return math.pow(r, 0.5)


# =================================================================================================================================
# CPU: the inputs have their properties
# =================================================================================================================================
def test_aran_sizes_sit_on_the_integers(oracle, refs):
    near, below, smallest = oc.aran_search()
    assert len(near) == 1692 and sorted(below) == sorted(oc.ARAN_TRUNCATED) and len(below) == 5
    assert smallest == oc.ARAN_LISTED_SMALLEST
    for k, (w, h) in enumerate(smallest, 1):
        assert abs(30.0 * math.sqrt(w / h) - k) < 1e-9
    assert [oc.aran_k(w, h) for (w, h) in oc.ARAN_TRUNCATED] == [25, 25, 25, 25, 12]
    for (w, h) in near:                                       # the device's sqrt and the reference's pow agree on every near-integer pair
        assert oc.aran_k(w, h) == oc.aran_k(w, h, _pow_root), (w, h)
    plane, boxes = _aran(refs)
    sizes = {(int(b[2]), int(b[3])) for b in boxes}
    for (w, h) in oc.ARAN_LISTED_SMALLEST + oc.ARAN_TRUNCATED + oc.ARAN_ZERO_EDGE:
        assert (w, h) in sizes and (h, w) in sizes
        assert oc.aran_k(w, h) == oc.aran_k(w, h, _pow_root) == oc.aran_k(h, w)
    assert (boxes[:, 0] >= 0).all() and (boxes[:, 1] >= 0).all() and (boxes[:, 0] + boxes[:, 2] <= oc.ARAN_SIDE).all() and (boxes[:, 1] + boxes[:, 3] <= oc.ARAN_SIDE).all()
    # (every pair near 26 or 13 is one of the five that truncate below: those two sizes are reached as 25 and 12 only)
    assert {oc.aran_k(int(b[2]), int(b[3])) for b in boxes} == set(range(0, 31)) - {26, 13}
    assert [oc.aran_k(w, h) for (w, h) in oc.ARAN_ZERO_EDGE] == [1, 1, 0, 0]
    q = refs.rows("aran", plane, boxes)
    for b, row in zip(boxes, q):
        assert row.any() == (oc.aran_k(int(b[2]), int(b[3])) > 0), b
    by_size = {(int(b[2]), int(b[3])): row for b, row in zip(boxes, q)}
    assert not by_size[(1, 901)].any() and not by_size[(901, 1)].any() and by_size[(1, 900)].any() and by_size[(900, 1)].any()


def test_form_boxes_reach_copy_and_exact_2x():
    b = oc.form_boxes()
    assert oc.FORM_W % 64 != 0 and oc.FORM_W % 2 == 1
    assert (b[:, 0] + b[:, 2] <= oc.FORM_W).all() and (b[:, 1] + b[:, 3] <= oc.FORM_H).all() and (b[:, :2] >= 0).all()
    mode = {(int(w), int(h)): oc.resize_mode(int(w), int(h)) for w, h in b[:, 2:]}
    # copy: the box is its own tile -- 30 x 30, and 29 x 30 / 30 x 29 too ((int)(30 sqrt(29 / 30)) = 29); exact 2 x: 60 x 60 alone
    assert {s for s, m in mode.items() if m == 0} == {(30, 30), (29, 30), (30, 29)} and {s for s, m in mode.items() if m == 1} == {(60, 60)}
    for s in (31, 59, 61):
        for t in (30, 60):
            assert mode[(s, t)] == 2 and mode[(t, s)] == 2
    assert {(1, 1), (1, 2), (2, 1), (2, 2), (oc.FORM_W, oc.FORM_H)} <= set(mode)
    for (w, h) in mode:
        at = {(int(x), int(y)) for x, y, ww, hh in b if (ww, hh) == (w, h)}
        assert at == {(0, 0), (oc.FORM_W - w, 0), (0, oc.FORM_H - h), (oc.FORM_W - w, oc.FORM_H - h)}


def test_content_cases_have_their_forms(oracle, refs):
    names, plane, boxes = oc.content_cases()
    assert plane.shape[1] <= 1920 and plane.shape[0] <= 1080 and len(names) == len(boxes)
    q = refs.rows("content", plane, boxes)
    maps = q.reshape(len(q), 8, 225)
    by = dict(zip(names, q))
    roi = {n: plane[b[1]:b[1] + b[3], b[0]:b[0] + b[2]] for n, b in zip(names, boxes)}
    # constant ROIs: 255 leaves nothing, everything else a full tile with marks on its own border only -- and both parities of 30 - k
    parities = set()
    for v in oc.CONST_VALUES:
        for (w, h) in oc.CONST_SIZES:
            n = f"const {v} {w}x{h}"
            assert oracle.otsu(roi[n], invert=True) == 0
            assert by[n].any() == (v != 255), n
            assert np.array_equal(by[n], by[f"const 0 {w}x{h}"]) or v == 255
            if w != h:
                parities.add((30 - oc.aran_k(w, h)) % 2)
    assert parities == {0, 1}
    full = by["const 0 30x30"].reshape(8, 15, 15)
    assert full[[0, 2, 4, 6]].any(axis=(1, 2)).all() and not full[[1, 3, 5, 7]].any()    # four straight runs along the tile's border, no diagonal step
    # maps that are entirely zero next to non-zero ones (mn == mx beside mn < mx), and a vector that is zero everywhere
    some, none_ = maps.any(axis=2), ~maps.any(axis=2)
    assert (some.any(axis=1) & none_.any(axis=1)).sum() > 20
    assert not by["shape single pixel"].any() and not by["shape single pixel in the corner"].any() and not by["const 255 30x30"].any()
    line = by["shape horizontal line"].reshape(8, 225).any(axis=1)
    assert line.tolist() == [True, False, False, False, True, False, False, False]
    assert by["shape diagonal"].reshape(8, 225).any(axis=1).tolist() == [False, True, False, False, False, True, False, False]
    assert by["shape checkerboard"].reshape(8, 225).any(axis=1).tolist() == [False, True] * 4
    assert by["shape ring"].reshape(8, 225).any(axis=1).all() and by["shape full tile with a hole"].reshape(8, 225).any(axis=1).all()
    for n, a in oc.shapes30().items():
        assert np.array_equal(roi["shape " + n], a) and roi["shape 2x " + n].shape == (60, 60)
    # the ramps: every grey level is there, the levels rotate by one from ROI to ROI while the threshold stays, and q moves with them
    for s in oc.RAMP_SHIFTS:
        r = roi[f"ramp {s}"]
        assert len(np.unique(r)) == 256 and (r[0] == r).all() and r[0, 0] == s
    assert len({oracle.otsu(roi[f"ramp {s}"], invert=True) for s in oc.RAMP_SHIFTS}) == 1
    moved = [s for s in oc.RAMP_SHIFTS[:-1] if not np.array_equal(by[f"ramp {s}"], by[f"ramp {s + 1}"])]
    assert len(moved) >= 2, moved                  # (the 30-wide tile taps two of every 8.5 columns of the 256: some one-column moves fall between)
    for side in (30, 60):                          # the raster ramps show a threshold one level off directly: copy and exact 2 x
        r = [by[f"raster ramp {side} {s}"] for s in oc.RASTER_SHIFTS]
        assert all(len(np.unique(roi[f"raster ramp {side} {s}"])) == 256 for s in oc.RASTER_SHIFTS)
        assert all(not np.array_equal(a, b) for a, b in zip(r, r[1:])), side
    # three levels with mirror-symmetric counts: the threshold is one of the two lower levels of 255 - roi, both answers occur, and the
    # answer is visible in q (the middle band is foreground, or it is not)
    forms, seen = set(), set()
    for (w, h) in oc.THREE_LEVEL_SIZES:
        forms.add(("one wave" if w <= 64 else "wide") + (", queued" if w * h > oc.OCR_BIG_PX else ""))
        per_th = {}
        for lv in oc.THREE_LEVELS:
            n = f"three-level {lv} {w}x{h}"
            r = roi[n]
            cnt = [int((r == v).sum()) for v in lv]
            assert cnt[0] == cnt[2] and cnt[1] > 0 and sum(cnt) == w * h
            inv = sorted(255 - v for v in lv)
            th = oracle.otsu(r, invert=True)
            assert th in inv[:2], (n, th)
            # (which of the two levels: the foreground is what lies above it, i.e. with the middle band or without)
            side = (inv.index(th), bool(lv[0] > lv[2]))
            seen.add(inv.index(th))
            per_th.setdefault(side, []).append(by[n])
        for rows in per_th.values():
            assert all(np.array_equal(rows[0], x) for x in rows[1:])
        if len({k[0] for k in per_th}) == 2:
            a, b = (per_th[k][0] for k in sorted(per_th) if not k[1])
            assert not np.array_equal(a, b)
    assert forms == {"one wave", "wide", "wide, queued"} and seen == {0, 1}
    assert {w for (w, _) in oc.THREE_LEVEL_SIZES} == {21, 64, 65, 257}


def test_slant_cases_reach_the_canvases_they_name(oracle, refs):
    plane = _slant(refs)
    cases = oc.slant_cases()
    assert set(cases) == {"switch", "steep", "fallback", "negative ch", "one wide or high"}
    differs = 0
    for name, (boxes, slopes) in cases.items():
        assert (boxes[:, 0] >= 0).all() and (boxes[:, 1] >= 0).all() and (boxes[:, 0] + boxes[:, 2] <= oc.SLANT_W).all() and (boxes[:, 1] + boxes[:, 3] <= oc.SLANT_H).all()
        for b, s in zip(boxes, slopes):
            w, h = int(b[2]), int(b[3])
            g = oc.rot_geom(w, h, float(s))
            assert 0 < g["rw"] * g["rh"] < oc.MAX_CANVAS
            assert g["on"] == (abs(s) > 0.01)
            if g["on"]:                                    # the restated geometry is the oracle's canvas
                roi = plane[b[1]:b[1] + h, b[0]:b[0] + w]
                rot = oracle.rotate_mat(roi, math.atan2(float(s), 1.0), crop=True)
                assert rot.shape == (g["rh"], g["rw"]), (name, b, s)
                if name == "fallback":
                    ch, full = oc.raw_crop_height(w, h, float(s))
                    assert full - 2 * ch <= 0 and g["crop"] == 0 and g["ch"] == 0 and s > 0
                    assert np.array_equal(rot, oracle.rotate_mat(roi, math.atan2(float(s), 1.0), crop=False))
                if name == "negative ch":
                    assert g["ch"] < 0 and g["rh"] > g["full_h"] and s < 0
                if name == "one wide or high":
                    assert g["rw"] == 1 or g["rh"] == 1
        q = refs.rows("slant", plane, boxes, slopes)
        q0 = refs.rows("slant", plane, boxes)
        differs += int((q != q0).any(axis=1).sum())
    assert differs > 50
    # the switch: 0.01 and the double below it are not rotated, the double above it is (src/OCR.cpp:73)
    sw = set(cases["switch"][1].tolist())
    assert {0.0, 0.01, -0.01, float(np.nextafter(0.01, 1)), float(np.nextafter(-0.01, -1)), float(np.nextafter(0.01, 0)), float(np.nextafter(-0.01, 0))} == sw
    assert oc.rot_geom(50, 40, 0.01)["on"] == 0 and oc.rot_geom(50, 40, float(np.nextafter(0.01, 1)))["on"] == 1 and oc.rot_geom(50, 40, float(np.nextafter(-0.01, -1)))["on"] == 1
    # steep slopes on every size from 1 x 1 to 160 x 160
    boxes, slopes = cases["steep"]
    assert set(np.abs(slopes).tolist()) == {0.8, 1.0, 1.5, 2.0, 5.0, 50.0} and (slopes > 0).sum() == (slopes < 0).sum()
    sizes = {(int(b[2]), int(b[3])) for b in boxes}
    assert {(1, 1), (160, 160), (1, 160), (160, 1), (1, 7), (7, 1)} <= sizes
    # the fall-back: the search's counts, and the listed shapes among what it finds
    f08, f15, f50 = oc.fallback_shapes(0.8), oc.fallback_shapes(1.5), oc.fallback_shapes(5.0)
    assert f08 == [(58, 1), (122, 1)] and len(f15) == 31 and len(f50) == 628 and {(7, 1), (7, 2), (8, 1)} <= set(f15)
    boxes, slopes = cases["fallback"]
    listed = {(int(b[2]), int(b[3]), float(s)) for b, s in zip(boxes, slopes)}
    assert {(58, 1, 0.8), (122, 1, 0.8)} <= listed
    assert len({k for k in listed if k[2] == 1.5}) == 5 and len({k for k in listed if k[2] == 5.0}) == 10
    assert all((k[0], k[1]) in set(f15) for k in listed if k[2] == 1.5) and all((k[0], k[1]) in set(f50) for k in listed if k[2] == 5.0)
    # negative crop heights: the two the issue names
    assert oc.rot_geom(100, 20, -5.0) == dict(on=1, crop=1, ch=-47, rw=39, rh=196, full_h=102)
    boxes, slopes = cases["negative ch"]
    assert {(100, 20, -0.5), (100, 20, -5.0)} <= {(int(b[2]), int(b[3]), float(s)) for b, s in zip(boxes, slopes)}
    boxes, slopes = cases["one wide or high"]
    g = [oc.rot_geom(int(b[2]), int(b[3]), float(s)) for b, s in zip(boxes, slopes)]
    assert any(x["rw"] == 1 and x["rh"] > 1 for x in g) and any(x["rh"] == 1 and x["rw"] > 1 for x in g) and any(x["rw"] == 1 and x["rh"] == 1 for x in g)
    # mixed waves: four different slopes in every group of four, rotated next to unrotated
    boxes, slopes = oc.mixed_wave_case()
    assert len(boxes) % oc.OCR_WAVES == 0 and len(boxes) >= 64
    for g0 in range(0, len(boxes), oc.OCR_WAVES):
        s = slopes[g0:g0 + oc.OCR_WAVES]
        on = np.abs(s) > 0.01
        assert len(set(s.tolist())) == oc.OCR_WAVES and on.any() and not on.all()
    assert (boxes[:, 0] + boxes[:, 2] <= oc.SLANT_W).all() and (boxes[:, 1] + boxes[:, 3] <= oc.SLANT_H).all()


def test_count_cases_straddle_the_workgroup_and_the_grid():
    boxes = oc.count_boxes()
    assert len(boxes) == oc.N_MANY > oc.FEATURE_WGS_PER_CU * oc.N_CU * oc.OCR_WAVES == 3072
    assert len({tuple(b) for b in boxes.tolist()}) == 31 and (boxes[:31] == boxes[31:62]).all()
    assert (boxes[:, 0] + boxes[:, 2] <= oc.FORM_W).all() and (boxes[:, 1] + boxes[:, 3] <= oc.FORM_H).all()
    for edge in (oc.OCR_WAVES, oc.OTSU_BLOCK, 4 * oc.OTSU_BLOCK):
        assert {edge - 1, edge, edge + 1} <= set(oc.COUNTS)
    assert 1 in oc.COUNTS and max(oc.COUNTS) < len(boxes)


@pytest.fixture(scope="module")
def list_oracle_cascades(oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("list_cascades")
    out = []
    for k, c in enumerate(oc.list_cascades()):
        p = d / f"list_{k}.classifier"
        p.write_text(c.text())
        out.append(oracle.cascade_load(str(p)))
    return tuple(out)


def _oracle_classes(oracle, planes, cascades, prm):
    """(classes in the library's candidate order -- plane by plane, ascending key --, ambiguous planes, pool sizes)"""
    cls, amb, sizes = [], [], []
    for p in planes:
        ref = oracle.detect_plane(p, cascades[0], cascades[1], **prm)
        order = np.argsort(ref["tree"].nodes[ref["pool"]]["key"], kind="stable") if len(ref["pool"]) else np.zeros(0, np.int64)
        cls.append(ref["cls"][order]); amb.append(int(ref["ambiguous"])); sizes.append(len(ref["pool"]))
    return np.concatenate(cls), amb, sizes


def test_list_batches_have_their_totals_and_class_patterns(oracle, list_oracle_cascades):
    chunk = oc.LIST_CHUNK
    totals = {}
    for name in oc.list_batches():
        planes, want = oc.list_planes(name)
        assert len(planes) <= 6 and planes.shape[1:] == (oc.LIST_H, oc.LIST_W)
        cls, amb, _ = _oracle_classes(oracle, planes, list_oracle_cascades, cc.RECT_PRM)
        assert np.array_equal(cls, want), name                  # every shape is pooled, in slot order, with the class it was made for
        assert not any(amb)
        assert len(cls) == oc.LIST_TOTALS[name]
        totals[name] = len(cls)
        on = cls > 0
        per_chunk = [on[i:i + chunk] for i in range(0, len(on), chunk)]
        if name == "none listed":
            assert not on.any() and len(on) > chunk
        elif name == "all listed":
            assert on.all() and len(on) > chunk and (cls == 1).any() and (cls == 2).any()
        elif name == "only the first":
            assert on[0] and on.sum() == 1 and len(per_chunk) == 3
        elif name == "only the last":
            assert on[-1] and on.sum() == 1 and len(per_chunk) == 3 and len(per_chunk[-1]) == 1
        elif name == "empty middle chunk":
            assert len(per_chunk) == 3 and per_chunk[0].any() and not per_chunk[1].any() and per_chunk[2].any()
        elif name != "1":
            for i in range(0, len(cls), chunk):                 # both classes, and pool-only candidates, in every chunk -- the partial last one included
                c = cls[i:i + chunk]
                assert (len(c) < 8) or ((c == 0).any() and (c == 1).any() and (c == 2).any()), (name, i)
    assert {totals[n] for n in ("1", "4095", "4096", "4097", "8192", "8193")} == {1, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1}
    assert totals["five chunks and more"] > 5 * chunk
    # the shapes' classes rest on bin 0 of the LBP histogram alone
    for k, (a, c) in oc.KINDS.items():
        b0 = oracle.lbp_hist(np.array(a, np.uint8))[0]
        assert (1 if b0 < 52 else 2 if b0 < 100 else 0) == c, (k, b0)


def test_tie_batch_is_ambiguous_with_more_than_256_candidates(oracle, oracle_cascades):
    planes = oc.tie_batch()
    cls, amb, sizes = _oracle_classes(oracle, planes, oracle_cascades, oc.TIE_PRM)
    assert all(a > 0 for a in amb) and all(n > 256 for n in sizes), (amb, sizes)
    off = 0
    for n in sizes:                                              # strong / weak candidates behind the lister's first pass of 256, pool-only ones everywhere
        c = cls[off:off + n]
        assert (c[256:] > 0).any() and (c[:256] == 0).any() and (c[256:] == 0).any()
        off += n


# =================================================================================================================================
# GPU
# =================================================================================================================================
def _check_q(f, refs, name, plane, boxes, slopes=None):
    want = refs.rows(name, plane, boxes, slopes)
    q = f.chain_run(plane, boxes, classify=False, slope=slopes)
    bad = np.flatnonzero((q != want).any(axis=1))
    assert len(bad) == 0, [(boxes[k].tolist(), None if slopes is None else float(np.broadcast_to(slopes, (len(boxes),))[k]), int((q[k] != want[k]).sum())) for k in bad[:8]]
    return q


@pytest.mark.gpu
def test_gpu_aran_target_sizes(erf, refs):
    """k = (int)(30 sqrt(R1)) on the device against (int)(30 pow(R1, 0.5)) where the product is an integer, truncates below one, or is 0."""
    plane, boxes = _aran(refs)
    q = _check_q(erf, refs, "aran", plane, boxes)
    assert not q[[k for k, b in enumerate(boxes) if max(b[2], b[3]) > 900 and min(b[2], b[3]) == 1]].any()
    _check_q(erf, refs, "aran", plane, boxes, np.zeros(len(boxes)))            # the same through the template branch chosen by rot[bi].on == 0


@pytest.mark.gpu
def test_gpu_resize_forms_at_the_corners(erf, refs):
    """Copy, exact 2 x and their neighbours at the four corners of a plane 333 pixels wide; 1 x 1 .. 2 x 2; the whole plane."""
    _check_q(erf, refs, "forms", _forms(refs), oc.form_boxes())


@pytest.mark.gpu
def test_gpu_content_forms(erf, refs):
    """Constant, two-level, three-level and ramp ROIs, and shapes whose marks lie on the tile's border or fill it."""
    names, plane, boxes = oc.content_cases()
    _check_q(erf, refs, "content", plane, boxes)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["switch", "steep", "fallback", "negative ch", "one wide or high"])
def test_gpu_slant(erf, refs, family):
    """RotSrc / make_rot_geom: slopes next to +-0.01, slopes up to +-50, the uncropped fall-back, canvases grown by a negative crop
    height, canvases one pixel wide or high."""
    boxes, slopes = oc.slant_cases()[family]
    _check_q(erf, refs, "slant", _slant(refs), boxes, slopes)


@pytest.mark.gpu
def test_gpu_slant_mixed_waves(erf, refs):
    """The four waves of a workgroup take different template branches and different canvases."""
    boxes, slopes = oc.mixed_wave_case()
    _check_q(erf, refs, "slant", _slant(refs), boxes, slopes)


@pytest.mark.gpu
def test_gpu_box_counts(erf, refs):
    """1 .. 257 boxes (four boxes a workgroup, 64 a k_ocr_otsu block), 3100 boxes (a second round of k_ocr_features' grid), then one again."""
    plane, boxes = _forms(refs), oc.count_boxes()
    first = _check_q(erf, refs, "forms", plane, boxes[:1])
    for n in oc.COUNTS:
        _check_q(erf, refs, "forms", plane, boxes[:n])
    _check_q(erf, refs, "forms", plane, boxes)
    assert np.array_equal(_check_q(erf, refs, "forms", plane, boxes[:1]), first)


@pytest.fixture(scope="module")
def svm_path(S, tmp_path_factory):
    p = tmp_path_factory.mktemp("ocr_edges_svm") / "ocr.model"
    p.write_bytes(gzip.open(S.cascade_io.ocr_model_path(5)).read())
    return str(p)


def _check_fused(S, f, planes, want_cls=None):
    """One fused call: every strong / weak candidate's (ocr_label, ocr_prob) == chain_run on its plane and box, every other one's (-1, 0)."""
    res = f.detect_planes(planes, S.STAGE_ALL | S.STAGE_OCR)
    c = res.cands
    assert res.ocr_label is not None and len(res.ocr_label) == len(c) == len(res.ocr_prob)
    if want_cls is not None:
        assert np.array_equal(c["cls"], want_cls)
    off = np.concatenate([[0], np.cumsum([p.n_pool for p in res.planes])])
    assert off[-1] == len(c) and len(res.planes) == len(planes)
    idle = c["cls"] == 0
    assert (res.ocr_label[idle] == -1).all() and (res.ocr_prob[idle] == 0).all()
    for k, plane in enumerate(planes):
        on = off[k] + np.flatnonzero(c["cls"][off[k]:off[k + 1]] > 0)
        if len(on) == 0:
            continue
        boxes = np.stack([c["x"][on], c["y"][on], c["w"][on], c["h"][on]], axis=1).astype(np.int32)
        _, label, prob = f.chain_run(plane, boxes)
        bad = np.flatnonzero((res.ocr_label[on] != label) | (res.ocr_prob[on] != prob))
        assert len(bad) == 0, (k, [(int(on[j]), int(res.ocr_label[on[j]]), int(label[j])) for j in bad[:8]])
        assert (label >= 0).all()
    return res


@pytest.fixture(scope="module")
def list_ctx(S, svm_path):
    f = S.ERFilter(params=S.Params(thresh_step=8, min_area=0, max_area=900000, stability_t=0, overlap_coef=0.7, max_width=oc.LIST_W,
                                   max_height=oc.LIST_H, max_frames=1))
    strong, weak = oc.list_cascades()
    f.load_cascade_text(0, strong.text())
    f.load_cascade_text(1, weak.text())
    f.load_svm_model(svm_path, 1800)
    yield f
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(oc.list_batches()))
def test_gpu_lister_against_the_box_path(S, list_ctx, name):
    """k_ocr_list's chunks: totals of 1, 4095 .. 4097, 8192, 8193 and 21000 candidates, nothing / everything / only the first / only the
    last listed, a whole chunk that lists nothing between two that do.  Twice on one context: the second call's scorer is enqueued behind
    classify, sized from the first."""
    planes, want = oc.list_planes(name)
    before = list_ctx.ocr_stage_stats()
    for _ in range(2):
        res = _check_fused(S, list_ctx, planes, want)
        assert len(res.cands) == oc.LIST_TOTALS[name]
    after = list_ctx.ocr_stage_stats()
    if (want > 0).any():                                         # (sized from this batch's own first call: the early scores are the ones returned)
        assert after["scored_early"] > before["scored_early"], (before, after)


@pytest.mark.gpu
def test_gpu_lister_after_a_tie_pass(S, cascade_paths, svm_path):
    """k_ocr_list_from: two noise planes whose NMS ties re-make their pools of about 800 candidates -- more than three passes of 256 --
    with the golden cascades (a few dozen strong / weak candidates among them)."""
    planes = oc.tie_batch()
    f = S.ERFilter(8, 6, 900000, 2, 0.3, max_width=oc.TIE_W, max_height=oc.TIE_H, max_frames=1)
    try:
        f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
        f.load_svm_model(svm_path, 1800)
        for _ in range(2):
            walked = f.tie_stats()["planes_walked"]
            res = _check_fused(S, f, planes)
            assert f.tie_stats()["planes_walked"] > walked
            assert all(p.ambiguous > 0 and p.n_pool > 256 for p in res.planes) and (res.cands["cls"] > 0).sum() > 10
        st = f.ocr_stage_stats()
        assert st["scored_early"] + st["scored_again"] >= 1, st
    finally:
        f.close()
