"""The premises of test_box_rounds.py, on the CPU: the batches pass two rounds of a capped grid, the cases are what they were made
for, a round that returned another case's result could not pass, the reservations stay small, and the repeated expectations have
the right lengths and agree with the references run on a short batch item by item."""
import itertools

import numpy as np

import box_round_cases as BC
import line_words_ref as LW


def _all_differ(items):
    return all(a != b for a, b in itertools.combinations(items, 2))


def test_cycle_and_batch():
    assert BC.K % 2 == 1 and BC.GRID_CAP % BC.K != 0 and BC.N > 2 * BC.GRID_CAP
    # the cases a workgroup takes in its rounds are different ones
    assert all(len({i % BC.K, (i + BC.GRID_CAP) % BC.K, (i + 2 * BC.GRID_CAP) % BC.K}) == 3 for i in range(BC.K))
    x = BC.extend([[1, 2], [3], [4, 5, 6]], 7)
    assert x.tolist() == [1, 2, 3, 4, 5, 6] * 2 + [1, 2]
    c, first = BC.starts([2, 1, 3], 7)
    assert c.tolist() == [2, 1, 3, 2, 1, 3, 2] and first.tolist() == [0, 2, 3, 6, 8, 9, 12]
    assert BC.extend([np.zeros((2, 4)), np.ones((1, 4))], 3).shape == (5, 4)


def test_mask_cases():
    plane, boxes = BC.mask_cases()
    assert plane.shape == (BC.MASK_H, BC.MASK_W) and len(boxes) == 2 * BC.K
    small, lds = boxes[0::2], boxes[1::2]
    assert [BC.mask_class(b[2], b[3]) for b in small] == [0] * BC.K and [BC.mask_class(b[2], b[3]) for b in lds] == [1] * BC.K
    assert BC.mask_class(64, 64) == 0 and BC.mask_class(65, 1) == 1 and BC.mask_class(128, 512) == 1 and BC.mask_class(128, 513) == 2
    assert (64, 64) in [(b[2], b[3]) for b in small] and len({b[3] for b in small}) >= 5
    assert all(65 <= b[2] <= 130 and 1 <= b[3] <= 16 for b in lds) and {(b[2] + 63) // 64 for b in lds} == {2, 3}
    assert {b[3] for b in lds} >= {1, 16} and [(b[2], b[3]) for b in lds] == list(BC.LDS_SIZES)
    for cls in (small, lds):
        assert sum(b[3] * ((b[2] + 31) // 32) for b in cls) <= BC.MASK_WORDS_MAX
    refs = BC.mask_refs()
    for part in (refs[0::2], refs[1::2]):                               # within a launch, every case's result differs from every other's
        assert _all_differ([(r[0].tobytes(), r[1]) for r in part])
        assert _all_differ([tuple(sorted((k, str(v)) for k, v in r[2].items())) for r in part])
        assert _all_differ([tuple(sorted(r[3].items())) for r in part])
    shapes = [r[2] for r in refs[0::2]]
    assert shapes[1]["euler"] == 0 and shapes[1]["hole_pixels"] == 9                        # the ring
    assert shapes[2]["euler"] == 0 and shapes[2]["hole_pixels"] == 2                        # the diagonal pair of hole pixels
    assert refs[6][1] == 2 and refs[10][1] == 17                                            # the diagonal pair of ink, the run up to the gap
    assert shapes[0]["hole_pixels"] > 0 and refs[0][3]["depth_max"] == 1                    # the 64 x 64 rings
    assert all(r[1] > b[2] for r, b in zip(refs[3::2], lds[1:])) and refs[1][1] == 34       # the floods go beyond the joining row
    assert set(np.unique(plane[plane != 255]).tolist()) == {0, 1, 2, 3} and (BC.LUT[:4] == 0).all() and BC.LUT[255] == 32


def test_mask_expectations_have_the_right_lengths():
    n = BC.N
    reg = BC.mask_regions()
    assert all(len(v) == 2 * n for v in reg.values())
    assert [BC.mask_class(w, h) for w, h in zip(reg["w"][:6], reg["h"][:6])] == [0, 1] * 3
    words, pixels = BC.mask_expected()
    assert len(pixels) == 2 * n and len(words) == int((reg["h"] * ((reg["w"] + 31) // 32)).sum())
    sh = BC.shape_expected()
    assert all(len(v) == 2 * n for v in sh.values()) and sh["crossings"].shape == (2 * n, 4)
    assert all(len(v) == 2 * n for v in BC.stroke_expected().values())
    # the tail of the batch: box 2 GRID_CAP + 4 of either class is case (2 GRID_CAP + 4) % K
    k = (2 * BC.GRID_CAP + 4) % BC.K
    refs = BC.mask_refs()
    assert pixels[-2] == refs[2 * k][1] and pixels[-1] == refs[2 * k + 1][1] and sh["hull_area2"][-1] == refs[2 * k + 1][2]["hull_area2"]


def test_feet_cases():
    geo, wds = BC.geom_cases(), BC.words_cases()
    assert len(geo) == len(wds) == BC.K
    for x, y, b in geo + wds:                                           # tight boxes inside the frame
        assert b[0].any() and b[-1].any() and b[:, 0].any() and b[:, -1].any()
        assert 0 <= x and x + b.shape[1] <= BC.FRAME_W and 0 <= y and y + b.shape[0] <= BC.FRAME_H
    hs = [b.shape[0] for _, _, b in geo]
    assert sum(2 * (h + 1) for h in hs) <= BC.GEOM_POINTS_MAX and min(hs) == 1 and max(hs) == 30
    ws = [b.shape[1] for _, _, b in wds]
    assert sum((w + 1) // 2 for w in ws) <= BC.WORD_RUNS_MAX and sorted(ws)[-2:] == [16, 130]
    g = BC.geom_refs()
    assert _all_differ([(tuple(sorted(r[0].items())), tuple(r[1]), tuple(r[2]), tuple(r[3])) for r in g])
    assert _all_differ([tuple(r[3]) for r in g]) and _all_differ([r[0]["m20"] for r in g])
    assert sorted(len(r[3]) for r in g)[0] == 4 and max(len(r[3]) for r in g) >= 6
    w = BC.words_refs()
    assert _all_differ([(r[0], tuple(r[1]), tuple(r[2])) for r in w])
    assert _all_differ([(len(r[2]), len(r[1]), r[0]) for r in w])                           # the line records alone differ as well
    assert {len(r[1]) for r in w} >= {1, 8} and all(1 <= len(r[1]) <= 8 for r in w)
    assert any(r0[0] < wds[0][0] + 64 < r0[1] for r0 in w[0][1])                            # a run across the word border of the wide case
    assert len(w[2][1]) == (ws[2] + 1) // 2                                                 # a case that fills its reserved slots


def test_feet_expectations_agree_with_the_references_item_by_item():
    n = 2 * BC.K + 4
    items = [BC.words_cases()[i % BC.K] for i in range(n)]
    ref = LW.tables(items)
    lines, runs, words = BC.words_expected(n)
    for got, want, names in ((lines, ref[0], ("first_word", "n_words", "first_run", "n_runs", "colmax", "reserved")),
                             (runs, ref[1], ("x0", "x1", "y0", "y1", "pixels", "word")),
                             (words, ref[2], ("line", "first_run", "n_runs", "x", "y", "w", "h", "pixels"))):
        assert [tuple(int(got[k][i]) for k in names) for i in range(len(want))] == want and all(len(got[k]) == len(want) for k in names)
    recs, bits = BC.feet_args(BC.words_cases(), n)
    assert all(len(v) == n for v in recs.values()) and len(bits) == int((recs["h"] * ((recs["w"] + 31) // 32)).sum())
    geoms, points = BC.geom_expected(n)
    refs = BC.geom_refs()
    assert len(points) == sum(len(refs[i % BC.K][3]) for i in range(n)) == int(geoms["count"].sum())
    for i in (0, BC.K - 1, BC.K, n - 1):
        a, c = int(geoms["first"][i]), int(geoms["count"][i])
        assert [tuple(p) for p in points[a:a + c].tolist()] == refs[i % BC.K][3] and geoms["qx"][i].tolist() == refs[i % BC.K][1]
    # the whole batch: the lengths
    lines, runs, words = BC.words_expected()
    assert len(lines["n_runs"]) == BC.N and len(runs["word"]) == int(lines["n_runs"].sum()) and len(words["line"]) == int(lines["n_words"].sum())
    assert int(runs["word"][-1]) == len(words["line"]) - 1 and int(words["line"][-1]) == BC.N - 1
    geoms, points = BC.geom_expected()
    assert len(geoms["first"]) == BC.N and geoms["qx"].shape == (BC.N, 4) and len(points) == int(geoms["first"][-1] + geoms["count"][-1])


def test_crop_cases(S):
    plane, lines = BC.crop_cases()
    assert plane.shape == (BC.CROP_PH, BC.CROP_PW) and plane.min() == 0 and plane.max() == 255 and len(lines) == BC.K
    refs = BC.crop_refs()
    assert _all_differ([g for g, _ in refs]) and _all_differ([b.tobytes() for _, b in refs])
    assert all(g[1] == 8 and 1 <= g[0] <= 16 and len(b) == 8 * g[0] for g, b in refs) and {g[0] for g, _ in refs} >= {1, 16}
    for (boxes, slope), (g, _) in zip(lines, refs):                     # the host's geometry is the numpy one, unit for unit
        rec = S.line_crop_geometry(np.asarray(boxes, np.int32), slope, height=8, max_width=16, pad=0.0)
        assert BC.CROP.fields(rec) == g
    boxes, first, count, slopes = BC.crop_args()
    assert len(first) == len(count) == len(slopes) == BC.N and len(boxes) == int(count.sum()) == int(first[-1] + count[-1])
    recs, pixels = BC.crop_expected()
    assert all(len(v) == BC.N for v in recs.values()) and len(pixels) == int((recs["width"] * recs["height"]).sum())
    assert int(recs["pix_off"][-1]) + int(recs["width"][-1]) * 8 == len(pixels)
