"""The per-box kernels past one round of their capped grids.  k_er_masks_small, k_er_masks_big<IN_LDS>, k_foot_geom, k_foot_words and
k_line_crops take one workgroup per box, at most 65536 of them, and walk on with `i += gridDim.x`; each test here sends
2 * 65536 + 5 boxes in one launch -- K = 9 hand-made cases in a cycle (box_round_cases.py) -- and holds every field of every box
against the references with ==, by whole-array comparison.  What a second round can get wrong: the loop step, the pointers derived
again per box, and the LDS the box before left behind (s_x, s_rows, s_occ / s_base / s_px / s_y0 / s_y1).

Left out, with the reason: the scratch class of the mask kernels (it keeps nothing in LDS between rounds, and 65537 such boxes need
about 1 GB of scratch); k_foot_pairs and k_foot_links (a second round needs more than 262144 lines, and each line walks every line of
the other set); k_text_map, k_run_tiles and k_run_cuts (the entry points that reach them build a tile and an 1800-byte feature row
per run)."""
import numpy as np
import pytest

import box_round_cases as BC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(S, cascade_paths):
    f = S.ERFilter(params=S.Params(max_width=640, max_height=480, max_frames=1, thresh_step=BC.STEP))
    f.load_cascade(0, cascade_paths[0])
    f.load_cascade(1, cascade_paths[1])
    yield f
    f.close()


def _same(got, want, what):
    """got == want element for element; a failure names the number of boxes that differ and the first of them."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want.astype(got.dtype)).reshape(len(got), -1).any(axis=1))[0] if len(got) else np.zeros(0, np.int64)
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} differ, the first at {bad[:8].tolist()}, the last at {int(bad[-1])}"


def _records(dtype, fields):
    n = len(next(iter(fields.values())))
    r = np.zeros(n, dtype)
    for k, v in fields.items():
        r[k] = v
    return r


@pytest.fixture(scope="module")
def regions(S, oracle):
    assert (oracle.quant_lut(BC.STEP) == BC.LUT).all()
    r = _records(S.CAND_DTYPE, BC.mask_regions())
    assert len(r) == 2 * BC.N > 4 * BC.GRID_CAP
    return BC.mask_cases()[0], r


def test_er_masks_two_rounds(ctx, regions):
    plane, r = regions
    words, pixels = ctx.er_masks(plane, r)
    want_words, want_pixels = BC.mask_expected()
    _same(pixels, want_pixels, "pixels")
    _same(words, want_words, "mask words")


def test_er_shapes_two_rounds(ctx, regions):
    plane, r = regions
    got = ctx.er_shapes(plane, r)
    for k, want in BC.shape_expected().items():
        _same(got[k], want, k)


def test_er_strokes_two_rounds(ctx, regions):
    plane, r = regions
    got = ctx.er_strokes(plane, r)
    for k, want in BC.stroke_expected().items():
        _same(got[k], want, k)


def test_feet_geom_two_rounds(S, ctx):
    recs, bits = BC.feet_args(BC.geom_cases())
    geoms, points = ctx.feet_geom(BC.FRAME_W, BC.FRAME_H, _records(S.LINE_FOOT_DTYPE, recs), bits)
    want, want_points = BC.geom_expected()
    assert len(geoms) == BC.N and set(want) == set(geoms.dtype.names)
    for k, v in want.items():
        _same(geoms[k], v, k)
    _same(points, want_points, "hull vertices")


def test_feet_words_two_rounds(S, ctx):
    recs, bits = BC.feet_args(BC.words_cases())
    got = ctx.feet_words(BC.FRAME_W, BC.FRAME_H, _records(S.LINE_FOOT_DTYPE, recs), bits)
    for name, table, want in zip(("line_words", "runs", "words"), got, BC.words_expected()):
        assert set(want) == set(table.dtype.names), name
        for k, v in want.items():
            _same(table[k], v, f"{name}.{k}")


def test_line_crops_two_rounds(ctx):
    plane, _ = BC.crop_cases()
    ctx.set_line_crop(*BC.CROP_SETTINGS)
    try:
        recs, pixels = ctx.line_crops(plane, *BC.crop_args())
    finally:
        ctx.set_line_crop()
    want, want_pixels = BC.crop_expected()
    assert len(recs) == BC.N and set(want) == set(recs.dtype.names)
    for k, v in want.items():
        _same(recs[k], v, k)
    _same(pixels, want_pixels, "crop bytes")
