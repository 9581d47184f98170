"""k_pyr_level (er_pyr_level.inl), the pyramid's own resize kernel, and launch_pyr_level's dispatch: bytes against oracle.resize through
str_er_pyr_level_plane, and the uniform-batch ingest that uses the dispatch for every level, plane trees against the oracle's at thresh step 1.

Every comparison is exact and against the oracle, never against a second run of the library.  The shape lists, and the restatement of the dispatch rule that
says which shapes must reach the new kernel, are in tests/test_pyr_level_rules.py, which also checks (without a GPU) that the lists reach the kernel's edges."""
import numpy as np
import pytest

from test_plane_builders import (FUSED_LEVELS, FUSED_MASK, _check_pyramid_planes, _first_difference, _resize_inputs, _step1_ctx, _thin_frame)
from test_pyr_level_rules import FALLBACK_SHAPES, PYRAMID_STEPS, ROWS, WIDTHS, _up4, heights, qualifies

gpu = pytest.mark.gpu


def _check(erf, oracle, sh, sw, sstride, dh, dw, dstride, rows, seed, expect_kernel):
    for name, src in _resize_inputs(sh, sw, seed):
        got, used = erf.pyr_level_plane(src, dw, dh, rows=rows, sstride=sstride, dstride=dstride)
        what = "(%d, %d) stride %d -> (%d, %d) stride %d, rows %d, %s" % (sh, sw, sstride, dh, dw, dstride, rows, name)
        assert used == expect_kernel, "%s: %s ran" % (what, "k_pyr_level" if used else "k_resize")
        d = _first_difference(got[None], oracle.resize(src, dw, dh)[None])
        assert d is None, "%s (%s): first difference at (x=%d, y=%d): got %d, expected %d (%d pixels differ)" % ((what, "k_pyr_level" if used else "k_resize") + d[1:])


@gpu
@pytest.mark.parametrize("rows", ROWS)
def test_every_width_and_height(erf, oracle, rows):
    """Forced tile height `rows`: dh in {1, rows - 1, rows, rows + 1, 2 rows + 3, 45} x dw in {255, 256, 257, 258, 259, 513}, sqrt(2) steps.  dh = 1 has no
    source height within (1, 1.5]: it is k_resize's, and says so; every other shape runs k_pyr_level."""
    for k, (sh, dh) in enumerate(heights(rows)):
        for sw, dw in WIDTHS:
            expect = qualifies(sh, sw, sw, dh, dw, _up4(dw))
            assert expect == (dh > 1)
            _check(erf, oracle, sh, sw, sw, dh, dw, _up4(dw), rows, 900 + 10 * rows + k, expect)


@gpu
def test_real_pyramid_steps(erf, oracle):
    """339 x 191 -> 240 x 135 -> 170 x 95 (the two smallest steps of a 1920 x 1080 pyramid) and the first step of a 1030-wide plane, rows padded to 64 bytes
    as in the plane pool, at the host's tile height and at every forced one."""
    for k, ((sh, sw, ss), (dh, dw, ds)) in enumerate(PYRAMID_STEPS):
        assert qualifies(sh, sw, ss, dh, dw, ds)
        for rows in (0,) + ROWS:
            _check(erf, oracle, sh, sw, ss, dh, dw, ds, rows, 950 + k, True)


@gpu
def test_dispatch_edges_fall_back_to_k_resize(erf, oracle):
    """Scale just above 1.5, an upscale, exact 2 x 2, a copy, a source stride that is no multiple of 4: k_resize runs, the bytes are the oracle's."""
    for k, ((sh, sw, ss), (dh, dw)) in enumerate(FALLBACK_SHAPES):
        _check(erf, oracle, sh, sw, ss, dh, dw, _up4(dw), 0, 970 + k, False)
    # ... and the same source as the last one at a stride that is one: the new kernel
    (sh, sw, _), (dh, dw) = FALLBACK_SHAPES[-1]
    _check(erf, oracle, sh, sw, 104, dh, dw, _up4(dw), 0, 975, True)


@gpu
@pytest.mark.parametrize("w,h", [(362, 204), (1030, 12)])
def test_uniform_batch_pyramid_at_step_1(S, cascade_paths, oracle, oracle_cascades, monkeypatch, w, h):
    """The batch path (ingest_uniform: plane and frame pitches, three planes a frame): text_detect on two frames, three levels, every plane's step-1 tree
    against oracle.pyramid of oracle.compute_channels.  Both levels of both sizes qualify for k_pyr_level (rows padded to 64 bytes)."""
    monkeypatch.delenv("STR_ER_PYR_KERNEL", raising=False)
    for l in range(1, FUSED_LEVELS):
        (sw, sh), (dw, dh) = oracle.pyr_dims(w, h, l - 1), oracle.pyr_dims(w, h, l)
        assert qualifies(sh, sw, (sw + 63) // 64 * 64, dh, dw, (dw + 63) // 64 * 64), (w, h, l)
    f = _step1_ctx(S, cascade_paths, max_width=w, max_height=h, max_frames=2, n_pyr_levels=FUSED_LEVELS, channel_mask=FUSED_MASK)
    try:
        frames = np.stack([_thin_frame(S, 740 + k, w, h) for k in range(2)])
        res = f.text_detect(frames, want_nodes=True)
        assert len(res.planes) == 2 * FUSED_LEVELS * 4
        _check_pyramid_planes(oracle, oracle_cascades, res, lambda i: oracle.compute_channels(frames[i]), FUSED_LEVELS, "text_detect %d x %d" % (w, h))
    finally:
        f.close()
