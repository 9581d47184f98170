"""OCR scorer, SVM half (config 3): svm_predict_probability.

The oracle (oracle/svm_oracle.c) is pinned bit for bit against the reference's own vendored libsvm
(oracle/_ref/libref_svm.so = src/svm.cpp compiled unmodified); tests/golden/svm_vectors.npz stores that
library's outputs so the comparison also works where /root/reference is absent.  The HIP path computes
the RBF kernel matrix with an f32 MFMA GEMM, so it is compared with the tolerance BASELINE.json states
for SVM scores (1e-4, absolute, on probabilities; labels must be equal)."""
import gzip
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-4


@pytest.fixture(scope="module")
def model_path(tmp_path_factory, S):
    p = tmp_path_factory.mktemp("svm") / "ocr_synth.model"
    p.write_bytes(gzip.open(S.cascade_io.ocr_model_path()).read())
    return str(p)


@pytest.fixture(scope="module")
def vectors():
    z = np.load(os.path.join(GOLDEN, "svm_vectors.npz"))
    return z["q"] / 255.0, z["label"], z["prob"], z["dec"]      # features are q/255.0 (src/OCR.cpp:211)


def test_oracle_matches_reference_vectors(oracle, model_path, vectors):
    from oracle.oracle import OracleSVM
    m = OracleSVM(oracle, model_path)
    assert (m.k, m.l) == (65, 319)
    x, lab, prob, dec = vectors
    for i in range(len(x)):
        l, p, d = m.predict_probability(x[i])
        assert l == lab[i] and np.array_equal(p, prob[i])
        if i < len(dec):
            assert np.array_equal(d, dec[i])
    assert abs(prob.sum(axis=1) - 1).max() < 1e-9


def test_oracle_matches_reference_library(oracle, model_path):
    from oracle.oracle import OracleSVM, RefSVM
    if not RefSVM.available():
        pytest.skip("oracle/_ref/libref_svm.so not present")
    m, r = OracleSVM(oracle, model_path), RefSVM(model_path)
    rng = np.random.default_rng(14)
    for _ in range(40):
        x = np.zeros(1800)
        nz = rng.choice(1800, size=int(rng.integers(0, 400)), replace=False)
        x[nz] = rng.integers(1, 256, len(nz)) / 255.0
        a, b = m.predict_probability(x), r.predict_probability(x)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.gpu
def test_gpu_svm_matches_reference_vectors(erf, model_path, vectors):
    erf.load_svm_model(model_path, 1800)
    assert erf.svm_info() == (65, 319, 1800)
    x, lab, prob, dec = vectors
    gl, gp, gd = erf.svm_predict_probability(x, want_dec=True)
    assert (gl == lab).all()
    assert np.abs(gp - prob).max() < TOL
    assert np.abs(gd[:len(dec)] - dec).max() < TOL
    assert np.abs(gp.sum(axis=1) - 1).max() < 1e-9


# ---- the model at the reference's training-set size (120 samples per class, src/utils.cpp:1478-1541): 4299 support vectors, up to 90 a class --------------
@pytest.fixture(scope="module")
def model120_path(tmp_path_factory, S):
    p = tmp_path_factory.mktemp("svm120") / "ocr_synth120.model"
    p.write_bytes(gzip.open(S.cascade_io.ocr_model_path(120)).read())
    return str(p)


@pytest.fixture(scope="module")
def vectors120():
    z = np.load(os.path.join(GOLDEN, "svm_vectors120.npz"))
    return z["q"] / 255.0, z["label"], z["prob"], z["dec"]


def test_oracle_matches_reference_vectors_120(oracle, model120_path, vectors120):
    """oracle/svm_oracle.c against what the reference's own libsvm returned for the 48 golden vectors on the big model: bit for bit."""
    from oracle.oracle import OracleSVM
    m = OracleSVM(oracle, model120_path)
    assert (m.k, m.l) == (65, 4299)
    x, lab, prob, dec = vectors120
    for i in range(len(x)):
        l, p, d = m.predict_probability(x[i])
        assert l == lab[i] and np.array_equal(p, prob[i])
        if i < len(dec):
            assert np.array_equal(d, dec[i])


@pytest.mark.gpu
def test_gpu_svm_matches_reference_vectors_120(S, model120_path, vectors120):
    """svm_predict_probability on the model of the reference's shape -- thousands of support vectors, the general (any count per class) build of
    k_svm_couple -- against the reference's libsvm: labels equal, probabilities and decision values within 1e-4."""
    f = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    f.load_svm_model(model120_path, 1800)
    assert f.svm_info() == (65, 4299, 1800)
    x, lab, prob, dec = vectors120
    gl, gp, gd = f.svm_predict_probability(x, want_dec=True)
    assert (gl == lab).all()
    assert np.abs(gp - prob).max() < TOL
    assert np.abs(gd[:len(dec)] - dec).max() < TOL
    assert np.abs(gp.sum(axis=1) - 1).max() < 1e-9
    f.close()


@pytest.mark.gpu
def test_gpu_chain_run_end_to_end_120(S, oracle, model120_path):
    """chain_run on real candidates with the big model (the box path: features as bf16 numerators, kernel matrix as three bf16 MFMAs) against the oracle."""
    from oracle.oracle import OracleSVM
    f = S.ERFilter(params=S.Params(max_width=640, max_height=480, max_frames=1))
    f.load_svm_model(model120_path, 1800)
    m = OracleSVM(oracle, model120_path)
    img = S.synth.gray(S.synth.stext_bgr(S.synth.frame_seed(6), 640, 480))
    res = f.detect_planes(img, S.STAGE_EXTRACT | S.STAGE_NMS)
    rng = np.random.default_rng(120)
    rnd = [(int(x), int(y), int(rng.integers(4, 640 - x + 1)), int(rng.integers(4, 480 - y + 1))) for x, y in zip(rng.integers(0, 600, 70), rng.integers(0, 440, 70))]
    boxes = np.concatenate([np.stack([res.cands["x"], res.cands["y"], res.cands["w"], res.cands["h"]], axis=1).astype(np.int32), np.array(rnd, np.int32)])
    assert len(boxes) > 70          # (more than 64: two groups of eight vectors per wave of k_svm_decide, and a ragged last one)
    q, label, prob = f.chain_run(img, boxes)
    for i, b in enumerate(boxes):
        l, p, _ = m.predict_probability(q[i] / 255.0)
        assert abs(prob[i] - p[np.argmax(p)]) < TOL
        top2 = np.sort(p)[-2:]
        if top2[1] - top2[0] > 10 * TOL:
            assert label[i] == l
    f.close()


@pytest.mark.gpu
def test_gpu_svm_matches_oracle_on_many(erf, oracle, model_path):
    from oracle.oracle import OracleSVM
    erf.load_svm_model(model_path, 1800)
    m = OracleSVM(oracle, model_path)
    rng = np.random.default_rng(15)
    n = 333                                                       # not a multiple of the 64-row GEMM tile
    x = np.zeros((n, 1800))
    for i in range(n):
        nz = rng.choice(1800, size=int(rng.integers(0, 600)), replace=False)
        x[i, nz] = rng.integers(1, 256, len(nz)) / 255.0
    gl, gp, gd = erf.svm_predict_probability(x, want_dec=True)
    for i in range(n):
        l, p, d = m.predict_probability(x[i])
        assert np.abs(gd[i] - d).max() < TOL and np.abs(gp[i] - p).max() < TOL
        top2 = np.sort(p)[-2:]
        if top2[1] - top2[0] > 10 * TOL:                          # skip near-ties of the arg max
            assert gl[i] == l


@pytest.mark.gpu
def test_gpu_svm_errors(S, model_path):
    f = S.ERFilter(8, 120, 900000, 2, 0.7, max_width=64, max_height=64, max_frames=1)
    with pytest.raises(S.StrErError) as e:
        f.svm_predict_probability(np.zeros((1, 1800)))
    assert e.value.code == -6
    with pytest.raises(S.StrErError) as e:
        f.load_svm_model("/nonexistent/OCR.model")            # reference: svm_load_model returns NULL
    assert e.value.code == -4
    with pytest.raises(S.StrErError) as e:
        f.load_svm_model(model_path, 100)                        # SV indices exceed the declared dimension
    assert e.value.code == -5
    f.load_svm_model(model_path, 1800)
    with pytest.raises(S.StrErError) as e:
        f.svm_predict_probability(np.zeros((1, 900)))
    assert e.value.code == -1
    f.close()


# ---- feature half (row a13): chain-code features; oracle restates the OpenCV primitives ("parity unpinned") ----
def test_oracle_chain_bitmaps_rectangle(oracle):
    """cv::findContours traces an outer border starting at its top-left pixel and going DOWN first."""
    img = np.zeros((30, 30), np.uint8)
    img[5:12, 8:20] = 255
    m = oracle.chain_bitmaps(img)
    assert [int((m[d] > 0).sum()) for d in range(8)] == [11, 0, 6, 0, 11, 0, 6, 0]
    assert (m[6][5:11, 8] == 255).all() and (m[4][11, 8:19] == 255).all()      # left edge: next point below; bottom: next to the right
    assert (m[2][6:12, 19] == 255).all() and (m[0][5, 9:20] == 255).all()      # right edge: next above; top: next to the left
    one = np.zeros((30, 30), np.uint8)
    one[3, 3] = 255
    assert oracle.chain_bitmaps(one).sum() == 0                                  # one-point contours are skipped (src/OCR.cpp:160)
    ring = np.zeros((30, 30), np.uint8)
    ring[4:20, 4:20] = 255
    ring[8:16, 8:16] = 0
    m = oracle.chain_bitmaps(ring)
    assert (m > 0).sum() == 60 + 32          # outer border 60 px + hole border 32 px (8-connected: it cuts the hole's corners)
    assert [int((m[d] > 0).sum()) for d in (1, 3, 5, 7)] == [1, 1, 1, 1]      # the four diagonal steps of the hole border


def test_oracle_otsu(oracle):
    img = np.concatenate([np.full(500, 40, np.uint8), np.full(300, 200, np.uint8)]).reshape(20, 40)
    t = oracle.otsu(img)
    assert 40 <= t < 200
    assert oracle.otsu(img, invert=True) == 255 - 200 or 55 <= oracle.otsu(img, invert=True) < 215


def test_oracle_rotate_mat(oracle):
    """OCR::rotate_mat (src/OCR.cpp:254-357): canvas size from the rounded corners, cropped by
    (int)((x2' - x1') * tan(rad) / 2) rows top and bottom; first row, last row and last column stay 0."""
    img = np.full((21, 41), 255, np.uint8)
    rad = float(np.arctan2(0.2, 1.0))
    full = oracle.rotate_mat(img, rad, crop=False)
    c, s = np.cos(rad), np.sin(rad)
    xs = [round(x * c - y * s) for x, y in ((-20, -10), (20, -10), (20, 10), (-20, 10))]
    ys = [round(x * s + y * c) for x, y in ((-20, -10), (20, -10), (20, 10), (-20, 10))]
    assert full.shape == (max(ys) - min(ys) + 1, max(xs) - min(xs) + 1)
    assert (full[-1] == 0).all() and (full[:, -1] == 0).all()                    # loops are exclusive (:292-295, :328-331)
    assert full[full.shape[0] // 2, full.shape[1] // 2] == 255                  # the centre maps into the source
    assert set(np.unique(full)) <= {0, 255}                                      # constant source: every bilinear tap is 255
    ch = int((xs[1] - xs[0]) * np.tan(rad) * 0.5)
    crop = oracle.rotate_mat(img, rad, crop=True)
    assert crop.shape == (full.shape[0] - 2 * ch, full.shape[1]) and ch > 0
    assert (crop[0] == 0).all()                                                  # i > min_y + crop_height (:301)
    # quirk kept: the source row is taken at (i - crop_height), so the cropped canvas shows the TOP rows of the
    # full canvas (rows 1 .. n-2), not its middle band
    assert (crop[1:-1] == full[1:crop.shape[0] - 1]).all()
    # negative angle: crop_height < 0 grows the canvas (kept as is)
    neg = oracle.rotate_mat(img, -rad, crop=True)
    assert neg.shape[0] > full.shape[0]
    # degenerate boxes still give a canvas (the uncropped fall-back of :285-289 needs 2*crop_height >= canvas height: flat boxes
    # at steep slopes get there -- 58x1 and 122x1 at slope 0.8, 31 shapes up to 160x160 at 1.5 -- see tests/test_ocr_edges.py)
    assert oracle.rotate_mat(np.full((1, 61), 255, np.uint8), float(np.arctan2(0.6, 1.0)), crop=True).shape[0] >= 1
    assert oracle.rotate_mat(np.full((1, 1), 255, np.uint8), 0.5, crop=True).shape == (1, 1)
    # interpolation: a half-plane edge produces intermediate grey levels
    half = np.zeros((31, 31), np.uint8)
    half[:, 16:] = 255
    r = oracle.rotate_mat(half, rad, crop=False)
    assert len(np.unique(r)) > 2
    # |slope| <= 0.01 is not rotated at all (:73)
    roi = np.random.default_rng(0).integers(0, 256, (40, 50), dtype=np.uint8)
    assert (oracle.ocr_normalise(roi, 0.01) == oracle.ocr_normalise(roi, 0.0)).all()
    assert (oracle.ocr_normalise(roi, 0.3) != oracle.ocr_normalise(roi, 0.0)).any()


@pytest.mark.gpu
def test_gpu_chain_features_rotated_match_oracle(erf, oracle, S):
    """chain_run with a text-line slope (src/OCR.cpp:73-78): rotate_mat sits between Otsu and ARAN."""
    img = S.synth.gray(S.synth.stext_bgr(S.synth.frame_seed(4), 640, 480))
    res = erf.detect_planes(img)
    boxes = np.stack([res.cands["x"], res.cands["y"], res.cands["w"], res.cands["h"]], axis=1).astype(np.int32)
    rng = np.random.default_rng(5)
    extra = []
    for _ in range(80):
        bw, bh = int(rng.integers(2, 160)), int(rng.integers(2, 160))
        extra.append((int(rng.integers(0, 640 - bw)), int(rng.integers(0, 480 - bh)), bw, bh))
    boxes = np.concatenate([boxes, np.array(extra + [(0, 0, 60, 60), (5, 5, 1, 1), (7, 7, 2, 1), (3, 3, 61, 5), (0, 0, 640, 480)], np.int32)])
    slopes = rng.uniform(-0.8, 0.8, len(boxes))
    slopes[::7] = 0.0
    slopes[1::7] = 0.01
    slopes[2::7] = -0.0101
    q = erf.chain_run(img, boxes, classify=False, slope=slopes)
    for b, sl, row in zip(boxes, slopes, q):
        exp = oracle.chain_features(img[b[1]:b[1] + b[3], b[0]:b[0] + b[2]], float(sl))
        assert (row == exp).all(), (b, sl)
    # one slope for the whole word, as er_ocr passes text.slope (src/ER.cpp:731)
    q1 = erf.chain_run(img, boxes[:10], classify=False, slope=0.25)
    for b, row in zip(boxes[:10], q1):
        assert (row == oracle.chain_features(img[b[1]:b[1] + b[3], b[0]:b[0] + b[2]], 0.25)).all()
    with pytest.raises(S.StrErError):
        erf.chain_run(img, boxes[:2], classify=False, slope=float("nan"))


@pytest.mark.gpu
def test_gpu_chain_features_match_oracle(erf, oracle, S):
    img = S.synth.gray(S.synth.stext_bgr(S.synth.frame_seed(4), 640, 480))
    res = erf.detect_planes(img)
    boxes = np.stack([res.cands["x"], res.cands["y"], res.cands["w"], res.cands["h"]], axis=1).astype(np.int32)
    rng = np.random.default_rng(3)
    extra = []
    for _ in range(60):
        bw, bh = int(rng.integers(2, 200)), int(rng.integers(2, 200))
        extra.append((int(rng.integers(0, 640 - bw)), int(rng.integers(0, 480 - bh)), bw, bh))
    boxes = np.concatenate([boxes, np.array(extra + [(0, 0, 60, 60), (5, 5, 1, 1), (0, 0, 640, 480)], np.int32)])
    q = erf.chain_run(img, boxes, classify=False)
    for b, row in zip(boxes, q):
        exp = oracle.chain_features(img[b[1]:b[1] + b[3], b[0]:b[0] + b[2]])
        assert (row == exp).all(), b
    assert (q > 0).any()


@pytest.mark.gpu
def test_gpu_chain_run_end_to_end(erf, oracle, S, model_path):
    """chain_run = features + svm_predict_probability; compared with oracle features fed to the oracle SVM."""
    from oracle.oracle import OracleSVM
    erf.load_svm_model(model_path, 1800)
    m = OracleSVM(oracle, model_path)
    img = S.synth.gray(S.synth.stext_bgr(S.synth.frame_seed(6), 640, 480))
    res = erf.detect_planes(img)
    c = res.cands[res.cands["cls"] > 0]
    boxes = np.stack([c["x"], c["y"], c["w"], c["h"]], axis=1).astype(np.int32)
    assert len(boxes) > 0
    q, label, prob = erf.chain_run(img, boxes)
    worst = 0.0
    for i, b in enumerate(boxes):
        l, p, _ = m.predict_probability(q[i] / 255.0)
        assert abs(prob[i] - p[np.argmax(p)]) < TOL
        worst = max(worst, abs(prob[i] - p[np.argmax(p)]))
        top2 = np.sort(p)[-2:]
        if top2[1] - top2[0] > 10 * TOL:
            assert label[i] == l
    # what the device path actually keeps (the tolerance above is BASELINE's): the kernel matrix through bf16 x 3 / f32 accumulation and the f32 pair table
    assert worst < 5e-6, worst


@pytest.mark.gpu
def test_gpu_config3_full_pipeline(S, cascade_paths, oracle, oracle_cascades, model_path):
    """BASELINE configs[2]: frames -> ER extract -> 2-stage classify -> chain-code + SVM on every strong/weak ER,
    all planes (inverted ones included) in one call; OCR outputs checked against the oracle per candidate."""
    from oracle.oracle import OracleSVM
    f = S.ERFilter(params=S.Params(max_width=640, max_height=480, max_frames=2))
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    f.load_svm_model(model_path, 1800)
    m = OracleSVM(oracle, model_path)
    frames = S.synth.frames_bgr("text", 20, 2, 640, 480)
    a = np.ascontiguousarray(frames)
    import ctypes as C
    rh = C.c_void_p()
    f._check(f.L.str_er_detect_bgr(f.h, a.ctypes.data, 640, 480, 3 * 640, 3 * 640 * 480, 2, 0, S.STAGE_ALL | S.STAGE_OCR, C.byref(rh)))
    res = f._collect(rh)
    assert res.ocr_label is not None and len(res.ocr_label) == len(res.cands)
    planes = [oracle.compute_channels(fr) for fr in frames]
    n_checked = 0
    for i, c in enumerate(res.cands):
        if c["cls"] == 0:
            assert res.ocr_label[i] == -1 and res.ocr_prob[i] == 0
            continue
        img = planes[int(c["frame"])][int(c["ch"])]
        q = oracle.chain_features(img[c["y"]:c["y"] + c["h"], c["x"]:c["x"] + c["w"]])
        l, p, _ = m.predict_probability(q / 255.0)
        assert abs(res.ocr_prob[i] - p.max()) < TOL
        top2 = np.sort(p)[-2:]
        if top2[1] - top2[0] > 10 * TOL:
            assert res.ocr_label[i] == l
        n_checked += 1
    assert n_checked > 10
    f.close()


@pytest.mark.gpu
def test_gpu_config3_full_pipeline_120(S, cascade_paths, oracle, model120_path):
    """The same at the reference's model size (120 samples a class, 4299 support vectors: k_svm_kernel_i8, k_svm_decide, k_svm_couple from the class sums),
    with the scorer enqueued behind classify: two calls, so that the second one is sized from the first and its early scores are the ones returned."""
    from oracle.oracle import OracleSVM
    f = S.ERFilter(params=S.Params(max_width=640, max_height=480, max_frames=1))
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    f.load_svm_model(model120_path, 1800)
    m = OracleSVM(oracle, model120_path)
    frames = S.synth.frames_bgr("text", 23, 2, 640, 480)
    n_checked = 0
    for fr in frames:
        res = f.text_detect(fr, S.STAGE_ALL | S.STAGE_OCR)
        assert res.ocr_label is not None and len(res.ocr_label) == len(res.cands)
        planes = oracle.compute_channels(fr)
        for i, c in enumerate(res.cands):
            if c["cls"] == 0:
                assert res.ocr_label[i] == -1 and res.ocr_prob[i] == 0
                continue
            img = planes[int(c["ch"])]
            q = oracle.chain_features(img[c["y"]:c["y"] + c["h"], c["x"]:c["x"] + c["w"]])
            l, p, _ = m.predict_probability(q / 255.0)
            assert abs(res.ocr_prob[i] - p.max()) < TOL
            top2 = np.sort(p)[-2:]
            if top2[1] - top2[0] > 10 * TOL:
                assert res.ocr_label[i] == l
            n_checked += 1
    assert n_checked > 20
    assert f.ocr_stage_stats()["scored_early"] >= 1
    f.close()


@pytest.mark.gpu
def test_gpu_ocr_stage_sized_on_the_device(S, cascade_paths, model_path, monkeypatch):
    """STAGE_OCR is enqueued behind classify, sized from the context's previous batch and working on the device's own count of strong / weak ERs
    (no read of the counters between classify and the scorer, like src/ER.cpp:728-735).  A sequence of batches -- few ERs, many more than guessed (scored
    again), the same again (early scores used), fewer, none, a batch in which an NMS tie pass re-makes the
    candidates of a plane after they were scored (only that plane is scored again) -- gives exactly what a context that sizes the scorer after reading the counters gives."""
    W, H = 1920, 1080
    def make():
        f = S.ERFilter(params=S.Params(max_width=W, max_height=H, max_frames=2, n_pyr_levels=8, channel_mask=0x07))
        f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
        f.load_svm_model(model_path, 1800)
        return f
    full = [S.synth.stext_bgr(S.synth.frame_seed(40 + i), W, H) for i in range(2)]
    few = np.full((H, W, 3), 128, np.uint8)
    few[300:460, 500:900] = full[0][300:460, 500:900]
    blank = np.full((H, W, 3), 90, np.uint8)
    ties = np.stack([S.synth.sties_bgr(S.synth.frame_seed(40), W, H), full[1]])       # (an NMS sibling tie that changes a pool: that plane's candidates are re-made)
    seq = [few[None], np.stack(full), np.stack(full), full[1][None], blank[None], full[0][None], ties, ties]
    stages = S.STAGE_ALL | S.STAGE_OCR
    f = make()
    got = [f.text_detect(a, stages) for a in seq]
    st = f.ocr_stage_stats()
    assert f.tie_stats()["planes_walked"] >= 2
    f.close()
    monkeypatch.setenv("STR_ER_OCR_SPEC", "0")
    g = make()
    want = [g.text_detect(a, stages) for a in seq]
    assert g.ocr_stage_stats() == {"scored_early": 0, "scored_again": 0}
    g.close()
    n = [int((r.cands["cls"] > 0).sum()) for r in want]
    assert n[0] >= 1 and n[1] > n[0] + n[0] // 8 + 256 + 128 and n[3] >= 1 and n[5] >= 1, n      # (the sequence exercises what it says)
    assert st["scored_again"] >= 3 and st["scored_early"] >= 3, st
    for a, b in zip(got, want):
        assert np.array_equal(a.cands, b.cands)
        assert np.array_equal(a.ocr_label, b.ocr_label) and np.array_equal(a.ocr_prob, b.ocr_prob)
        assert ((a.ocr_label >= 0) == (a.cands["cls"] > 0)).all()


@pytest.mark.gpu
def test_gpu_line_ocr_stage(S, cascade_paths, oracle, model_path):
    """er_ocr's first half (src/ER.cpp:695-747) on the lines of er_grouping: chain_run with the line's slope on every member's
    (merged) bound, the 0.95-overlap deletion, MIN_OCR_PROB, min_pass_ocr -- restated here over the oracle's pieces."""
    from oracle.oracle import OracleSVM
    W, H, F = 640, 480, 2
    f = S.ERFilter(8, 120, 900000, 2, 0.7, 0.15, max_width=W, max_height=H, max_frames=F)
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    f.load_svm_model(model_path, 1800)
    f.set_min_ocr_prob(0.05)
    m = OracleSVM(oracle, model_path)
    frames = np.stack([S.synth.stext_bgr(S.synth.frame_seed(40 + i), W, H) for i in range(F)])
    st = S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP | S.GROUP_INNER_SUP | S.STAGE_OCR_LINES
    res = f.text_detect(frames, st)
    assert res.line_label is not None and len(res.line_label) == len(res.text_ers) > 0 and res.times[5] > 0
    planes = [oracle.compute_channels(fr) for fr in frames]
    n_rot = 0
    for t, tx in enumerate(res.texts):
        mem = res.text_ers[tx["first"]:tx["first"] + tx["count"]]
        boxes = res.group_bounds[mem]
        probs = []
        for j, (ci, g) in enumerate(zip(mem, boxes)):
            c = res.cands[ci]
            roi = planes[c["frame"]][c["ch"]][g["y"]:g["y"] + g["h"], g["x"]:g["x"] + g["w"]]
            q = oracle.chain_features(roi, float(tx["slope"]))
            n_rot += abs(tx["slope"]) > 0.01
            l, p, _ = m.predict_probability(q / 255.0)
            pmax = p[np.argmax(p)]
            k = tx["first"] + j
            assert abs(res.line_prob[k] - pmax) < TOL
            top2 = np.sort(p)[-2:]
            if top2[1] - top2[0] > 10 * TOL:
                assert res.line_label[k] == l
            probs.append(res.line_prob[k])
        # the two deletions and min_pass_ocr, as the reference does them
        n = len(mem)
        dele = [False] * n
        for a in range(n):
            for b in range(a + 1, n):
                A, B = boxes[a], boxes[b]
                iw = min(A["x"] + A["w"], B["x"] + B["w"]) - max(A["x"], B["x"])
                ih = min(A["y"] + A["h"], B["y"] + B["h"]) - max(A["y"], B["y"])
                inter = float(iw * ih) if iw > 0 and ih > 0 else 0.0
                uni = float((max(A["x"] + A["w"], B["x"] + B["w"]) - min(A["x"], B["x"])) * (max(A["y"] + A["h"], B["y"] + B["h"]) - min(A["y"], B["y"])))
                if inter / uni > 0.95:
                    if int(A["w"]) * int(A["h"]) > int(B["w"]) * int(B["h"]):
                        dele[b] = True
                    else:
                        dele[a] = True
        keep = [not dele[a] and not (probs[a] < 0.05) for a in range(n)]
        assert list(res.line_kept[tx["first"]:tx["first"] + tx["count"]]) == keep
        assert bool(res.text_alive[t]) == (sum(keep) >= 2)
    assert n_rot > 0            # some line is slanted enough to go through rotate_mat
    with pytest.raises(S.StrErError):
        f.text_detect(frames, S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_OCR_LINES)
    f.close()


# ---- the direction marks as a function of the 8-neighbour mask (k_ocr_features: chain_lut) ----
def _chain_lut():
    """Python statement of chain_lut (scene-text-recognition_amd/csrc/ocr_kernels.hip): bit c of lut[nb] = direction code c is marked at a
    foreground pixel whose neighbours are nb (bit d of nb = neighbour d, counter-clockwise from east)."""
    lut = np.zeros(256, np.uint8)
    for nb in range(256):
        out = 0
        for b in range(8):
            if not (nb >> b) & 1:
                continue
            swept4, dn = False, b
            for s in range(b + 1, b + 9):
                if (nb >> (s & 7)) & 1:
                    dn = s & 7
                    break
                if s % 2 == 0:
                    swept4 = True
            if swept4:
                out |= 1 << ((4 - dn) & 7)
        lut[nb] = out
    return lut


def _marks_from_masks(img, lut):
    ddx, ddy = [1, 1, 0, -1, -1, -1, 0, 1], [0, -1, -1, -1, 0, 1, 1, 1]
    f = np.zeros((32, 32), np.uint8)
    f[1:31, 1:31] = img > 0
    nb = np.zeros((30, 30), np.int64)
    for d in range(8):
        nb |= f[1 + ddy[d]:31 + ddy[d], 1 + ddx[d]:31 + ddx[d]].astype(np.int64) << d
    o = np.where(f[1:31, 1:31] > 0, lut[nb], 0)
    return np.stack([((o >> c) & 1).astype(np.uint8) * 255 for c in range(8)])


def test_direction_marks_are_a_function_of_the_neighbour_mask(oracle):
    """The border tracer (cv::findContours restated in the oracle, one pixel at a time) and the per-pixel table the GPU
    uses mark the same (pixel, direction) pairs: on every 3x3 neighbourhood and on random, blob-like and thin images."""
    lut = _chain_lut()
    for nb in range(256):                                       # every neighbourhood, in the middle of an empty image
        img = np.zeros((30, 30), np.uint8)
        img[10, 10] = 255
        for d, (dx, dy) in enumerate(zip([1, 1, 0, -1, -1, -1, 0, 1], [0, -1, -1, -1, 0, 1, 1, 1])):
            if (nb >> d) & 1:
                img[10 + dy, 10 + dx] = 255
        assert np.array_equal(oracle.chain_bitmaps(img), _marks_from_masks(img, lut)), nb
    rng = np.random.default_rng(77)
    for trial in range(400):
        kind = trial % 4
        if kind == 0:
            img = (rng.random((30, 30)) < rng.uniform(0.05, 0.95)).astype(np.uint8) * 255
        elif kind == 1:                                          # blobs with holes
            img = np.zeros((30, 30), np.uint8)
            for _ in range(int(rng.integers(1, 6))):
                x0, y0 = rng.integers(0, 25, 2); w, h = rng.integers(1, 12, 2); img[y0:y0 + h, x0:x0 + w] = 255
            for _ in range(int(rng.integers(0, 4))):
                x0, y0 = rng.integers(0, 28, 2); w, h = rng.integers(1, 5, 2); img[y0:y0 + h, x0:x0 + w] = 0
        elif kind == 2:                                          # one-pixel strokes, diagonals, image borders
            img = np.zeros((30, 30), np.uint8)
            for _ in range(int(rng.integers(1, 8))):
                x, y = rng.integers(0, 30, 2); dx, dy = rng.integers(-1, 2, 2)
                for _ in range(int(rng.integers(2, 30))):
                    if 0 <= x < 30 and 0 <= y < 30:
                        img[y, x] = 255
                    x, y = x + dx, y + dy
        else:                                                    # foreground values other than 255
            img = (rng.random((30, 30)) < 0.5).astype(np.uint8) * int(rng.integers(1, 256))
        assert np.array_equal(oracle.chain_bitmaps(img.copy()), _marks_from_masks(img, lut)), trial


# ---- models with other class counts: the coupling kernel has builds for k <= 64, k = 65 and k - 1 > 64 coefficient columns, the first two each for
# "at most 5 support vectors a class" (registers) and for any count (in eights) ----
def _synthetic_model(path, k, dim, rng, empty_class=None, nsv_max=6):
    """A libsvm text model (svm_save_model format) with random support vectors / coefficients (1 .. nsv_max per class, some class has nsv_max);
    class `empty_class` has no support vector."""
    nsv = [int(rng.integers(1, nsv_max + 1)) for _ in range(k)]
    nsv[k // 2] = nsv_max
    if empty_class is not None:
        nsv[empty_class] = 0
    l, npairs = sum(nsv), k * (k - 1) // 2
    with open(path, "w") as f:
        f.write("svm_type c_svc\nkernel_type rbf\ngamma 0.05\n")
        f.write(f"nr_class {k}\ntotal_sv {l}\n")
        f.write("rho " + " ".join(f"{v:.6g}" for v in rng.normal(0, 0.5, npairs)) + "\n")
        f.write("label " + " ".join(str(i) for i in range(k)) + "\n")
        f.write("probA " + " ".join(f"{v:.6g}" for v in rng.uniform(-3, -0.5, npairs)) + "\n")
        f.write("probB " + " ".join(f"{v:.6g}" for v in rng.normal(0, 0.3, npairs)) + "\n")
        f.write("nr_sv " + " ".join(str(v) for v in nsv) + "\nSV\n")
        for _ in range(l):
            coefs = " ".join(f"{v:.6g}" for v in rng.normal(0, 2.0, k - 1))
            idx = np.sort(rng.choice(dim, size=int(rng.integers(1, dim // 2)), replace=False))
            f.write(coefs + " " + " ".join(f"{i}:{rng.integers(1, 256) / 255.0:.6g}" for i in idx) + " \n")
    return l


@pytest.mark.gpu
@pytest.mark.parametrize("k,empty,nsv_max", [(2, None, 6), (7, 3, 6), (64, None, 6), (66, 0, 6), (100, 99, 6),
                                             (2, None, 5), (7, 0, 5), (33, 32, 5), (64, 5, 5), (65, 64, 6), (65, 0, 13), (40, None, 19), (65, 7, 3)])
def test_gpu_svm_other_class_counts(S, oracle, tmp_path, k, empty, nsv_max):
    from oracle.oracle import OracleSVM
    rng = np.random.default_rng(1000 + k + 7 * nsv_max)
    dim = 96
    path = str(tmp_path / f"k{k}.model")
    l = _synthetic_model(path, k, dim, rng, empty, nsv_max)
    f = S.ERFilter(8, 120, 900000, 2, 0.7, max_width=64, max_height=64, max_frames=1)
    f.load_svm_model(path, dim)
    assert f.svm_info() == (k, l, dim)
    m = OracleSVM(oracle, path)
    n = 70
    x = np.zeros((n, dim))
    for i in range(n):
        nz = rng.choice(dim, size=int(rng.integers(0, dim)), replace=False)
        x[i, nz] = rng.integers(1, 256, len(nz)) / 255.0
    gl, gp, gd = f.svm_predict_probability(x, want_dec=True)
    for i in range(n):
        lab, p, d = m.predict_probability(x[i])
        assert np.abs(gd[i] - d).max() < TOL and np.abs(gp[i] - p).max() < TOL, (k, i)
        top2 = np.sort(p)[-2:]
        if k == 2 or top2[1] - top2[0] > 10 * TOL:
            assert gl[i] == lab
    assert np.abs(gp.sum(axis=1) - 1).max() < 1e-9
    f.close()
