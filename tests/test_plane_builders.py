"""The kernels that build the planes everything else is computed from -- k_bgr_to_ycrcb, k_nv12_to_ycrcb, k_resize and their list forms
(er_planes.inl) -- pixel for pixel against the oracle, at the tile and form edges of each.

Every comparison is exact.  Where a plane can be read back (compute_channels, resize_plane) its bytes are compared; where it cannot (NV12
ingest, the pyramid inside text_detect*, lists, the stream) the plane's component tree at thresh_step 1 and min_area 0 is: at step 1 every grey
level is a tree level and every node is kept, so one pixel off by one level changes the area of some node.  The reference is always the oracle
(oracle.compute_channels / nv12_to_ycrcb / resize / pyramid), never a second run of the library.

Without a GPU two tests run: a numpy restatement of cv::resize's 8-bit INTER_LINEAR against oracle.resize on the shape list of the GPU test (the
reference of that test is then stated twice, independently), and a restatement of k_resize's form selection that keeps the shape list honest."""
import math

import numpy as np
import pytest

from conftest import check_plane_against_oracle

gpu = pytest.mark.gpu


def _first_difference(got, ref):
    """None, or (plane, x, y, got, expected, count) of the first differing pixel of two (planes, h, w) arrays."""
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.uint8, (got.shape, ref.shape)
    if got.tobytes() == ref.tobytes():
        return None
    ne = got != ref
    k, y, x = (int(v) for v in np.argwhere(ne)[0])
    return k, x, y, int(got[k, y, x]), int(ref[k, y, x]), int(ne.sum())


def _assert_same_planes(got, ref, what):
    d = _first_difference(got, ref)
    assert d is None, "%s: plane %d differs first at (x=%d, y=%d): got %d, expected %d (%d pixels differ)" % ((what,) + d)


# ======================================================================================================================================
# k_resize: the form a tile takes (restated from resize_tile_body.inl), the shape list, cv::resize restated in numpy
# ======================================================================================================================================
RS_WORDS, RS_ROWS = 96, 16          # er_planes.inl: the LDS window of a tile, dwords x rows
RESIZE_ROWS, TILE_W = 8, 256        # a tile of the output: 64 lanes x 4 columns, 8 rows
TABLE_FORMS = ("fast", "byte", "global")

#                 source (h, w)  destination (h, w)
RESIZE_SHAPES = [((24, 724), (17, 512)),
                 ((24, 724), (17, 513)),
                 ((12, 520), (12, 519)),
                 ((12, 516), (13, 517)),
                 ((30, 768), (20, 512)),
                 ((20, 400), (20, 267)),
                 ((40, 100), (60, 300)),       # upscale across a tile edge
                 ((20, 396), (20, 263)),       # scale_x just above 1.5: global on the full tile, staged byte taps on the partial one
                 ((30, 772), (20, 514)),
                 ((40, 800), (27, 530)),
                 ((20, 400), (9, 258)),
                 ((24, 728), (15, 456)),       # staged byte taps on 200 columns of the second tile
                 ((20, 320), (13, 200)),       # ... and on the first (and only) tile of a narrow plane
                 ((34, 1200), (16, 520)),      # global on two full tiles
                 ((40, 102), (60, 301)),       # a source stride that is no multiple of 4: nothing is staged
                 ((16, 1032), (8, 516)),       # exact 2x2
                 ((16, 1030), (8, 515)),
                 ((12, 600), (12, 600))]       # copy


def _scales(sh, sw, dh, dw):
    return 1.0 / (dw / sw), 1.0 / (dh / sh)          # (host_resize_geom: the doubles cv::resize computes)


def _resize_mode(sh, sw, dh, dw):
    if (dh, dw) == (sh, sw):
        return "copy"
    scale_x, scale_y = _scales(sh, sw, dh, dw)
    eps = float(np.finfo(np.float64).eps)
    isx, isy = round(scale_x), round(scale_y)         # (rint: half to even, like round())
    if abs(scale_x - isx) < eps and abs(scale_y - isy) < eps and isx == 2 and isy == 2:
        return "2x2"
    return "linear"


def _tap(d, scale):
    return int(math.floor(np.float32((d + 0.5) * scale - 0.5)))


def resize_tile_forms(sh, sw, dh, dw, sstride=None):
    """The form every tile of k_resize / k_resize_list takes: [(tile x, tile y, form, straddles)], form one of copy / 2x2 / fast (staged in LDS,
    dword reads and byte permutes, scale_x <= 1.5) / byte (staged, byte taps) / global (taps from global memory).  `straddles`: the tile is
    staged, its window reaches the plane's last row, and the last dword of the window holds bytes beyond the row's last pixel.

    A restatement of the selection rule of resize_tile_body.inl (x_lo, x_hi, y_lo, y_hi, nwords, nrows, staged, the 1.5 split) for
    test_resize_shape_list_reaches_every_form: it guards the COVERAGE of the shape list, not the kernel's correctness, and has to follow
    RS_WORDS, RS_ROWS and the rule if they change.  The plane's first pixel is taken to be dword-aligned (it is, in every buffer of the library);
    sstride defaults to sw, which is what str_er_resize_plane passes."""
    sstride = sw if sstride is None else sstride
    mode = _resize_mode(sh, sw, dh, dw)
    scale_x, scale_y = _scales(sh, sw, dh, dw)
    out = []
    for ty in range((dh + RESIZE_ROWS - 1) // RESIZE_ROWS):
        for tx in range(((dw + 3) // 4 + 63) // 64):
            if mode != "linear":
                out.append((tx, ty, mode, False))
                continue
            tx0, dy0 = tx * TILE_W, ty * RESIZE_ROWS
            sx = lambda dx: min(max(_tap(dx, scale_x), 0), sw - 1)
            x_lo = sx(tx0) & ~3
            x_last = sx(min(tx0 + TILE_W - 1, dw - 1))
            x_hi = x_last + 1 if x_last + 1 < sw else x_last
            y_lo = min(max(_tap(dy0, scale_y), 0), sh - 1)
            y_hi = min(max(_tap(min(dy0 + RESIZE_ROWS - 1, dh - 1), scale_y) + 1, 0), sh - 1)
            nwords, nrows = (x_hi - x_lo) // 4 + 1, y_hi - y_lo + 1
            staged = nwords <= RS_WORDS and nrows <= RS_ROWS and sstride % 4 == 0
            form = ("fast" if scale_x <= 1.5 else "byte") if staged else "global"
            out.append((tx, ty, form, staged and y_hi == sh - 1 and x_lo + 4 * nwords > sw))
    return out


def cv_resize_linear_u8(src, dw, dh):
    """OpenCV 4.x cv::resize(8UC1, INTER_LINEAR) in plain numpy: the same-size copy, the exact 2x2 decimation (which takes INTER_AREA's path),
    otherwise the float32 coefficient tables in 2048 fixed point (INTER_RESIZE_COEF_BITS = 11), a horizontal pass into int32 and the vertical
    pass ((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2 >> 2.  Written from OpenCV's resize.cpp, not from oracle/er_oracle.c."""
    src = np.ascontiguousarray(src, dtype=np.uint8)
    sh, sw = src.shape
    mode = _resize_mode(sh, sw, dh, dw)
    if mode == "copy":
        return src.copy()
    s = src.astype(np.int32)
    if mode == "2x2":
        return ((s[0:2 * dh:2, 0:2 * dw:2] + s[0:2 * dh:2, 1:2 * dw:2] + s[1:2 * dh:2, 0:2 * dw:2] + s[1:2 * dh:2, 1:2 * dw:2] + 2) >> 2).astype(np.uint8)
    scale_x, scale_y = _scales(sh, sw, dh, dw)

    def table(n, scale):
        f = ((np.arange(n, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
        i = np.floor(f).astype(np.int64)
        return i, f - i.astype(np.float32)                                   # (float32 arithmetic throughout)

    def coef(f):
        one, k = np.float32(1.0), np.float32(2048.0)
        return np.rint((one - f) * k).astype(np.int32), np.rint(f * k).astype(np.int32)      # cvRound: half to even

    x, fx = table(dw, scale_x)
    fx = np.where((x < 0) | (x >= sw - 1), np.float32(0.0), fx).astype(np.float32)
    x = np.clip(x, 0, sw - 1)
    x1 = np.minimum(x + 1, sw - 1)
    a0, a1 = coef(fx)
    y, fy = table(dh, scale_y)
    b0, b1 = coef(fy)
    y0, y1 = np.clip(y, 0, sh - 1), np.clip(y + 1, 0, sh - 1)
    r0 = s[y0][:, x] * a0 + s[y0][:, x1] * a1
    r1 = s[y1][:, x] * a0 + s[y1][:, x1] * a1
    v = (((b0[:, None] * (r0 >> 4)) >> 16) + ((b1[:, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def _resize_inputs(sh, sw, seed):
    """The planes a shape is resized from: noise; a one-pixel checkerboard of 0 and 255 (the largest products, the clamp at 255); a single 255
    in each corner (a tap on the wrong side of an edge shows)."""
    yy, xx = np.mgrid[0:sh, 0:sw]
    corners = np.zeros((sh, sw), np.uint8)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = 255
    return [("noise", np.random.default_rng(seed).integers(0, 256, (sh, sw), dtype=np.uint8)),
            ("checkerboard", (((xx + yy) & 1) * 255).astype(np.uint8)),
            ("corners", corners)]


def test_resize_shape_list_reaches_every_form(capsys):
    """Coverage guard (see resize_tile_forms): every form of k_resize is reached by the shape list, each of the three table forms also on a tile
    beyond the first of a row (x_lo > 0, base - x_lo, the window's last word) and on a first tile; the list holds every dw % 4, both kinds of
    source width, a last tile row that is not full, exact 2x2 and copy beyond one tile.  Prints which shape reaches which form on which tile."""
    reached = {}
    for (sh, sw), (dh, dw) in RESIZE_SHAPES:
        for tx, ty, form, _ in resize_tile_forms(sh, sw, dh, dw):
            reached.setdefault((form, tx > 0), {}).setdefault(((sh, sw), (dh, dw)), set()).add(tx)
    with capsys.disabled():
        print()
        for (form, beyond), shapes in sorted(reached.items()):
            print("k_resize form %-6s %s: %s" % (form, "x-tile > 0" if beyond else "x-tile 0  ",
                                                   ", ".join("%s->%s tiles %s" % (s, d, sorted(t)) for (s, d), t in shapes.items())))
    for form in TABLE_FORMS:
        assert (form, False) in reached and (form, True) in reached, form
    assert ("2x2", True) in reached and ("copy", True) in reached
    linear = [(s, d) for s, d in RESIZE_SHAPES if _resize_mode(s[0], s[1], d[0], d[1]) == "linear"]
    assert {d[1] % 4 for _, d in linear} == {0, 1, 2, 3}
    assert {s[1] % 4 == 0 for s, _ in linear} == {True, False}
    assert any(d[0] % RESIZE_ROWS for _, d in linear)
    assert any(d[1] < s[1] for s, d in linear) and any(d[1] > s[1] for s, d in linear)        # reductions and an upscale


def test_cv_resize_restated_in_numpy_equals_the_oracle(oracle):
    """The reference of test_resize_every_form, stated twice: oracle.resize (C, a pixel at a time) and cv_resize_linear_u8 (numpy, from
    OpenCV's resize.cpp) agree byte for byte on every shape and input of that test, and on the small shapes of tests/test_gpu_parity.py."""
    small = [((108, 192), (76, 136)), ((52, 52), (26, 26)), ((9, 200), (26, 5)), ((200, 9), (8, 26)), ((3, 3), (26, 26)), ((1, 1), (7, 5))]
    for k, ((sh, sw), (dh, dw)) in enumerate(RESIZE_SHAPES + small):
        for name, src in _resize_inputs(sh, sw, 500 + k):
            _assert_same_planes(cv_resize_linear_u8(src, dw, dh)[None], oracle.resize(src, dw, dh)[None],
                                "(%d, %d) -> (%d, %d), %s: numpy restatement (got) against the oracle" % (sh, sw, dh, dw, name))


@gpu
def test_resize_every_form(erf, oracle):
    """k_resize through resize_plane against oracle.resize, byte for byte: every form, on first and later x-tiles (RESIZE_SHAPES)."""
    for k, ((sh, sw), (dh, dw)) in enumerate(RESIZE_SHAPES):
        forms = resize_tile_forms(sh, sw, dh, dw)
        for name, src in _resize_inputs(sh, sw, 500 + k):
            d = _first_difference(erf.resize_plane(src, dw, dh)[None], oracle.resize(src, dw, dh)[None])
            if d is not None:
                _, x, y, got, exp, n = d
                form = [f for tx, ty, f, _ in forms if (tx, ty) == (x // TILE_W, y // RESIZE_ROWS)][0]
                pytest.fail("(%d, %d) -> (%d, %d), %s: first difference at (x=%d, y=%d), tile (%d, %d), form %s: got %d, expected %d (%d pixels differ)"
                            % (sh, sw, dh, dw, name, x, y, x // TILE_W, y // RESIZE_ROWS, form, got, exp, n))


# ======================================================================================================================================
# k_bgr_to_ycrcb
# ======================================================================================================================================
CUBE_STEP = 0x9E3779        # odd: i -> i * CUBE_STEP mod 2^24 is a permutation; its bytes 0x79, 0x37, 0x9E move all three channels from pixel to pixel


def _cube_frame(k):
    """Quarter k of the 2^24 BGR triples as a 2048 x 2048 frame.  Pixel i holds the triple whose bytes are (B, G, R) = i * CUBE_STEP mod 2^24:
    any two of the four pixels of a quad differ in all three channels (by 1, 2 or 3 times 0x79 / 0x37 / 0x9E plus a carry, never 0 mod 256)."""
    i = np.arange(k << 22, (k + 1) << 22, dtype=np.uint64)
    t = (i * np.uint64(CUBE_STEP)) & np.uint64(0xFFFFFF)
    return np.stack([t & np.uint64(255), (t >> np.uint64(8)) & np.uint64(255), t >> np.uint64(16)], axis=-1).astype(np.uint8).reshape(2048, 2048, 3)


def test_cube_order_visits_every_triple_once():
    """The order of _cube_frame is a permutation of the 2^24 triples, and the pixels of a quad differ in every channel."""
    assert math.gcd(CUBE_STEP, 1 << 24) == 1
    q = _cube_frame(3).reshape(-1, 4, 3).astype(np.int32)
    for a in range(4):
        for b in range(a + 1, 4):
            assert (q[:, a, :] != q[:, b, :]).all()


@gpu
def test_compute_channels_whole_bgr_cube(S, oracle):
    """All 2^24 BGR triples through k_bgr_to_ycrcb's dword path (w % 4 == 0: every colour goes through the packed Cr / Cb stores), six planes
    each, against oracle.compute_channels: four frames of 2048 x 2048 through a context of exactly that size."""
    f = S.ERFilter(params=S.Params(max_width=2048, max_height=2048, max_frames=1))
    try:
        for k in range(4):
            frame = _cube_frame(k)
            _assert_same_planes(f.compute_channels(frame), oracle.compute_channels(frame), "quarter %d of the BGR cube" % k)
    finally:
        f.close()


@gpu
def test_compute_channels_byte_path_and_row_tails(erf, oracle):
    """Widths around the 1024 pixels one workgroup converts of a row, and the smallest ones: a width that is no multiple of 4 takes the byte
    path on every pixel; 1020 / 1024 / 1028 end a row on the dword path in the first / at the end of the first / in the second workgroup."""
    rng = np.random.default_rng(11)
    for w in (1, 2, 3, 5, 1020, 1021, 1022, 1023, 1024, 1025, 1027, 1028, 2049):
        for h in (1, 3):
            for name, frame in (("noise", rng.integers(0, 256, (h, w, 3), dtype=np.uint8)),
                                ("0 / 255", (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8))):
                _assert_same_planes(erf.compute_channels(frame), oracle.compute_channels(frame), "%d x %d, %s" % (w, h, name))


# ======================================================================================================================================
# planes without a read-back: the tree at thresh_step 1, min_area 0
# ======================================================================================================================================
def _step1_ctx(S, cascade_paths, **kw):
    f = S.ERFilter(params=S.Params(thresh_step=1, min_area=0, **kw))
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    return f


def _check_step1(oracle, oracle_cascades, p, img, what):
    assert (p.height, p.width) == img.shape, what
    try:
        check_plane_against_oracle(oracle, p, img, oracle_cascades, step=1, min_area=0)
    except AssertionError as e:
        raise AssertionError("%s, frame %d, channel %d, level %d (%d x %d): the plane's step-1 tree is not the oracle's" %
                             (what, p.frame, p.ch, p.pyr, p.width, p.height)) from e


def _check_pyramid_planes(oracle, oracle_cascades, res, three_of_frame, n_levels, what):
    """Every plane of a result against oracle.pyramid of the frame's three planes [Y, Cr, Cb] (255 - x for the inverted channels 3 .. 5)."""
    pyr = {}
    for p in res.planes:
        if (p.frame, p.ch % 3) not in pyr:
            pyr[(p.frame, p.ch % 3)] = oracle.pyramid(three_of_frame(p.frame)[p.ch % 3], n_levels)
        img = pyr[(p.frame, p.ch % 3)][p.pyr]
        _check_step1(oracle, oracle_cascades, p, 255 - img if p.ch >= 3 else img, what)


@gpu
def test_nv12_ingest_planes(S, cascade_paths, oracle, oracle_cascades):
    """k_nv12_to_ycrcb: the three planes of frames of independent random bytes (U and V unrelated: a Cr / Cb swap or a wrong chroma row shows),
    two frames a call (frame pitch), widths on both sides of a workgroup's 1024 pixels and of a quad, against oracle.nv12_to_ycrcb."""
    f = _step1_ctx(S, cascade_paths, max_width=1030, max_height=6, max_frames=2)
    rng = np.random.default_rng(21)
    try:
        for w in (2, 4, 6, 1022, 1024, 1026, 1030):
            for h in (2, 6):
                nv = rng.integers(0, 256, (2, h + h // 2, w), dtype=np.uint8)
                res = f.text_detect_nv12(nv, w, h, want_nodes=True)
                assert [(p.frame, p.ch) for p in res.planes] == [(fr, c) for fr in range(2) for c in range(6)]
                for p in res.planes:
                    img = oracle.nv12_to_ycrcb(nv[p.frame], w, h)[p.ch % 3]
                    _check_step1(oracle, oracle_cascades, p, 255 - img if p.ch >= 3 else img, "NV12 %d x %d" % (w, h))
        # str_er_detect_nv12 takes even sizes only ("NV12 frames have even width and height"): an odd height is an error, not a rounded-down frame
        with pytest.raises(S.StrErError) as e:
            f.text_detect_nv12(rng.integers(0, 256, (3 + 1, 4), dtype=np.uint8), 4, 3)
        assert e.value.code == -1 and "even" in str(e.value)
    finally:
        f.close()


def _thin_frame(S, seed, w, h):
    """An S-text frame with a little noise on top: every 256-column tile of every plane holds many distinct levels, yet far fewer step-1 nodes
    than a frame of pure noise."""
    rng = np.random.default_rng(seed)
    return np.clip(S.synth.stext_bgr(S.synth.frame_seed(seed), w, h).astype(np.int32) + rng.integers(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)


LIST_SIZES = [(1030, 12), (516, 20), (258, 9)]          # (w, h): 5, 3 and 2 tiles a row at level 0; 3, 2 and 1 at level 1
FUSED_LEVELS, FUSED_MASK = 3, 0x0F                      # Y, Cr, Cb and the inverted Y


def test_fused_frames_cross_tile_edges(oracle):
    """Coverage guard for the step-1 tests of the fused path (the planes' rows are padded to 64 bytes there, so every tile is staged and a
    sqrt(2) step takes the fast form): their pyramid levels have tiles beyond the first of a row, and at least one source width is no multiple
    of 4, so that the last dword of a window on the last row holds bytes beyond the row's last pixel."""
    beyond = straddles = 0
    for w0, h0 in LIST_SIZES + [(518, 10)]:
        for l in range(1, FUSED_LEVELS):
            (sw, sh), (dw, dh) = oracle.pyr_dims(w0, h0, l - 1), oracle.pyr_dims(w0, h0, l)
            tiles = resize_tile_forms(sh, sw, dh, dw, sstride=(sw + 63) // 64 * 64)
            assert {t[2] for t in tiles} == {"fast"}, (w0, h0, l)
            beyond += sum(t[0] > 0 for t in tiles)
            straddles += sum(t[3] for t in tiles)
    assert beyond >= 8 and straddles >= 2, (beyond, straddles)


@gpu
def test_list_builders_at_step_1(S, cascade_paths, oracle, oracle_cascades):
    """k_bgr_to_ycrcb_list and k_resize_list (the job-table search, tiles beyond the first of a row): three BGR frames of different sizes in one
    text_detect_list call, three pyramid levels, every plane against oracle.pyramid of oracle.compute_channels."""
    f = _step1_ctx(S, cascade_paths, max_width=1030, max_height=20, max_frames=3, n_pyr_levels=FUSED_LEVELS, channel_mask=FUSED_MASK)
    try:
        frames = [_thin_frame(S, 700 + k, w, h) for k, (w, h) in enumerate(LIST_SIZES)]
        res = f.text_detect_list(frames, want_nodes=True)
        assert [(p.frame, p.pyr, p.ch) for p in res.planes] == [(fr, l, c) for fr in range(3) for l in range(FUSED_LEVELS) for c in range(4)]
        _check_pyramid_planes(oracle, oracle_cascades, res, lambda i: oracle.compute_channels(frames[i]), FUSED_LEVELS, "text_detect_list")
    finally:
        f.close()


@gpu
def test_nv12_list_builders_at_step_1(S, cascade_paths, oracle, oracle_cascades):
    """k_nv12_to_ycrcb_list and k_resize_list: two NV12 frames of different sizes in one text_detect_nv12_list call."""
    f = _step1_ctx(S, cascade_paths, max_width=1030, max_height=12, max_frames=2, n_pyr_levels=FUSED_LEVELS, channel_mask=FUSED_MASK)
    try:
        sizes = [(1030, 12), (518, 10)]
        nv = [S.synth.nv12_from_bgr(_thin_frame(S, 710 + k, w, h)) for k, (w, h) in enumerate(sizes)]
        res = f.text_detect_nv12_list(nv, want_nodes=True)
        assert len(res.planes) == 2 * FUSED_LEVELS * 4
        _check_pyramid_planes(oracle, oracle_cascades, res, lambda i: oracle.nv12_to_ycrcb(nv[i], *sizes[i]), FUSED_LEVELS, "text_detect_nv12_list")
    finally:
        f.close()


@gpu
def test_uniform_batch_builders_at_step_1(S, cascade_paths, oracle, oracle_cascades):
    """k_bgr_to_ycrcb and k_resize with plane and frame pitches: text_detect on two frames of 1030 x 12, three levels."""
    f = _step1_ctx(S, cascade_paths, max_width=1030, max_height=12, max_frames=2, n_pyr_levels=FUSED_LEVELS, channel_mask=FUSED_MASK)
    try:
        frames = np.stack([_thin_frame(S, 720 + k, 1030, 12) for k in range(2)])
        res = f.text_detect(frames, want_nodes=True)
        assert len(res.planes) == 2 * FUSED_LEVELS * 4
        _check_pyramid_planes(oracle, oracle_cascades, res, lambda i: oracle.compute_channels(frames[i]), FUSED_LEVELS, "text_detect")
    finally:
        f.close()


@gpu
def test_stream_list_builders_at_step_1(S, cascade_paths, oracle, oracle_cascades):
    """One list submission on the ingest stream, the frames at odd offsets and odd row strides in the staging buffer (as in
    tests/test_ragged_stream.py): the unaligned path of the fused ingest.  The records are the blocking list call's, the planes the oracle's."""
    prm = S.Params(thresh_step=1, min_area=0, max_width=1040, max_height=24, max_frames=3, n_pyr_levels=FUSED_LEVELS, channel_mask=FUSED_MASK)
    st = S.FrameStream(prm, depth=1)
    ref = S.ERFilter(params=prm)
    try:
        for c in (st, ref):
            c.load_cascade(0, cascade_paths[0]); c.load_cascade(1, cascade_paths[1])
        frames = [_thin_frame(S, 730 + k, w, h) for k, (w, h) in enumerate(LIST_SIZES)]
        slot, buf = st.acquire()
        layout, at = [], 0
        for k, fr in enumerate(frames):
            h, w = fr.shape[:2]
            stride = 3 * w + 5 + 2 * k
            at += 1 + 2 * k                         # frame k starts 1 + 2 k bytes after the end of the one before: odd offsets
            for y in range(h):
                buf[at + y * stride:at + y * stride + 3 * w] = fr[y].reshape(-1)
            layout.append((at, w, h, stride))
            at += (h - 1) * stride + 3 * w
        assert all(s % 2 == 1 for _, _, _, s in layout) and layout[0][0] % 2 == 1
        st.submit_list(slot, layout, S.STAGE_ALL | S.WANT_NODES)
        _, got = st.next()
        exp = ref.text_detect_list(frames, want_nodes=True)
        assert got.info.tobytes() == exp.info.tobytes() and got.cands.tobytes() == exp.cands.tobytes()
        for a, b in zip(got.planes, exp.planes):
            assert a.nodes.tobytes() == b.nodes.tobytes()
        _check_pyramid_planes(oracle, oracle_cascades, got, lambda i: oracle.compute_channels(frames[i]), FUSED_LEVELS, "stream submit_list")
    finally:
        st.close(); ref.close()
