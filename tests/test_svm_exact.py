"""The OCR scorer's SVM half against an exact reference (tests/svm_exact.py): decision values within a bound derived from each form's arithmetic,
full probability vectors, across the forms the loader picks (bytes / bf16x3, class sums or not, k_svm_couple's MODE 0 / 1 / 2 and MSV 5 / 0 / -1),
and the box path (chain_run) tied to svm_predict_q8 bit for bit."""
import gzip
import os

import numpy as np
import pytest

import svm_exact as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# Probabilities: the device keeps the pairwise table in f32 and steps the coupling with the hardware's 24-bit reciprocal (DESIGN 3.7 estimates 1e-8 to
# 1e-7 from these); P_TOL is that estimate with a margin, not a fitted number.
P_TOL = 1e-6
# A vector whose reference coupling evaluates its stopping statistic (max_t |Qp_t - pQp| against 0.005 / k) within MARGIN of the threshold may stop one
# sweep earlier or later on the device; such vectors are left out of the probability check and counted, at most MAX_EXCLUDED of a case's vectors (the
# issue's 2 %; every case scores 1000 vectors besides its tile-shaped batch so that the share is measured on enough of them).  How far the device's
# statistic can be from the reference's: the pairwise table holds e = f32(r_ij) (|de| <= 2^-25 for r <= 1) and uses 1 - e for r_ji, so an off-diagonal
# Q_tj = -e (1 - e) moves by at most 2^-25 and Q_tt = sum_j r_jt^2 by 2^-24 sum_j r_jt; with sum p = 1 and p_t sum_j r_jt <= 1 (at the uniform start
# (k - 1) / k, and smaller as the iterate settles), Qp_t and pQp each move by at most 2^-25 + 2^-24, the statistic by 2^-23.  The coupling's step
# divides by the hardware's 24-bit reciprocal (a relaxation factor 1 +- 2^-23): another 2^-23.  MARGIN = 2 x that sum.
MARGIN = 2.0 * (2.0 ** -23 + 2.0 ** -23)
MAX_EXCLUDED = 0.02
N_MORE = 1000
STATS = {}


def _ctx(S):
    return S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))


def check_scores(m, osvm, q, gl, gp, gd, path="q8", name=""):
    """Every decision value within its bound; probabilities within P_TOL + max|probA| / 4 x the vector's largest bound (vectors whose coupling
    stops within MARGIN of its threshold excluded and counted: the caller asserts MAX_EXCLUDED over its case); labels equal where the reference's top two differ by more than twice that tolerance."""
    K, dK = m.kernel(q, path)
    dec, bound = m.decision(K, dK)
    ratio = np.abs(gd - dec) / bound
    bad = np.argwhere(ratio > 1.0)
    assert len(bad) == 0, (name, bad[:5].tolist(), np.abs(gd - dec)[tuple(bad[0])], bound[tuple(bad[0])])
    lab, prob, sweeps, margin = E.couple(osvm, dec)
    ptol = P_TOL + np.abs(m.probA).max() / 4 * bound.max(axis=1)
    keep = margin >= MARGIN
    excluded = int((~keep).sum())
    perr = np.abs(gp - prob).max(axis=1)
    assert (perr[keep] <= ptol[keep]).all(), (name, np.argwhere(perr > ptol)[:5].ravel().tolist(), perr.max(), ptol.min())
    top = np.sort(prob, axis=1)
    clear = keep & (top[:, -1] - top[:, -2] > 2 * ptol)          # (an excluded vector may take one sweep more or less: its probabilities move by more)
    assert (gl[clear] == lab[clear]).all(), name
    if (m.label == np.arange(m.k)).all():
        assert np.array_equal(gp[np.arange(len(q)), gl], gp.max(axis=1))        # pv[label] is the arg max's entry
    key = (path if path != "q8" else ("bytes" if m.bytes else "bf16x3"), m.class_sums, m.mode)
    s = STATS.setdefault(key, [0.0, 0.0, 0, 0])
    s[0] = max(s[0], float(ratio.max())); s[1] = max(s[1], float((perr[keep] / ptol[keep]).max()) if keep.any() else 0.0)
    s[2] += excluded; s[3] += len(q)
    return K, excluded


def assert_excluded(excluded, n, name):
    assert excluded <= MAX_EXCLUDED * n, (name, excluded, n)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, (r, pr, ex, n) in sorted(STATS.items(), key=str):
        print(f"\nsvm exact: form {k}: max |d dec| / bound {r:.3g}, max |d prob| / tol {pr:.3g}, excluded {ex} of {n}")


def _shipped(S, tmp_path_factory, per_class):
    raw = gzip.open(S.cascade_io.ocr_model_path(per_class)).read()
    p = tmp_path_factory.mktemp(f"svm{per_class}") / "ocr.model"
    p.write_bytes(raw)
    return str(p), E.Model(raw, 1800)


# (name, k, lo, hi, empty classes, total mod 64, top count, dim, n)
CASES = [
    ("k2_msv5_d1", 2, 1, 4, (), None, 5, 1, 1),
    ("k7_sums_d1800", 7, 9, 14, (3,), 1, None, 1800, 129),
    ("k64_msv0_d127", 64, 6, 8, (0,), 63, None, 127, 65),
    ("k64_sums_d1800", 64, 9, 13, (63,), 0, None, 1800, 128),
    ("k65_sums_d1800", 65, 9, 21, (64,), 0, None, 1800, 1000),
    ("k65_msv0_d1800", 65, 6, 8, (), 1, None, 1800, 200),
    ("k65_msv5_d200", 65, 1, 4, (0,), 63, 5, 200, 127),
    ("k66_d128", 66, 1, 12, (0,), 1, None, 128, 64),
    ("k100_d129", 100, 1, 9, (99,), 0, None, 129, 63),
]


@pytest.mark.gpu
@pytest.mark.parametrize("byte", [True, False], ids=["bytes", "bf16x3"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gpu_q8_synthetic_forms(S, oracle, tmp_path, case, byte):
    from oracle.oracle import OracleSVM
    name, k, lo, hi, empty, l_mod, top, dim, n = case
    rng = np.random.default_rng(7000 + 13 * k + dim + (0 if byte else 1))
    nsv = E.class_counts(rng, k, lo, hi, empty, l_mod, top)
    text, svb = E.synth_model(rng, nsv, dim, byte)
    path = tmp_path / "m.model"
    path.write_bytes(text)
    m = E.Model(text, dim)
    # the form the loader must pick for this case
    assert m.bytes == byte
    want = {"k2_msv5_d1": (False, 0, 5), "k7_sums_d1800": (True, 0, -1), "k64_msv0_d127": (False, 0, 0), "k64_sums_d1800": (True, 0, -1),
            "k65_sums_d1800": (True, 1, -1), "k65_msv0_d1800": (False, 1, 0), "k65_msv5_d200": (False, 1, 5), "k66_d128": (False, 2, 0),
            "k100_d129": (False, 2, 0)}[name]
    assert (m.class_sums, m.mode, m.msv_build) == want, (name, m.form())
    if l_mod is not None:
        assert sum(nsv) % 64 == l_mod
    if m.class_sums:
        assert {c % 4 for c in nsv if c} >= {1, 2, 3}, nsv            # (k_svm_decide's fourth-rounded last step with 1, 2 and 3 live ranks)
    f = _ctx(S)
    try:
        f.load_svm_model_text(text, dim)
        assert f.svm_info() == (k, sum(nsv), dim)
        assert f.svm_forms() == {"bytes": byte, "class_sums": m.class_sums}
        osvm = OracleSVM(oracle, str(path))
        q = E.near_vectors(rng, svb, n)
        gl, gp, gd = f.svm_predict_q8(q, want_dec=True)
        K, ex = check_scores(m, osvm, q, gl, gp, gd, "q8", name)
        if n >= 20:
            assert (K.max(axis=1) > 0.1).mean() > 0.6, name              # (not a comparison of rho with itself)
        q2 = E.near_vectors(rng, svb, N_MORE)
        gl, gp, gd = f.svm_predict_q8(q2, want_dec=True)
        K, ex2 = check_scores(m, osvm, q2, gl, gp, gd, "q8", name)
        assert (K.max(axis=1) > 0.1).mean() > 0.6, name
        assert_excluded(ex + ex2, n + N_MORE, name)
        if name in ("k7_sums_d1800", "k66_d128"):
            # the double-input path (f32 k_svm_kernel) on the same vectors, with the f32 bound
            gl2, gp2, gd2 = f.svm_predict_probability(q2 / 255.0, want_dec=True)
            _, ex = check_scores(m, osvm, q2, gl2, gp2, gd2, "f64", name)
            assert_excluded(ex, N_MORE, name)
    finally:
        f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("per_class", [5, 120])
def test_gpu_q8_shipped_models(S, oracle, tmp_path_factory, per_class):
    """The two shipped models (both in the byte form: MSV 5 and the class sums, MODE 1), on vectors near their support vectors, on the golden vectors
    (against the reference and against the reference's own libsvm outputs), and on random ones."""
    from oracle.oracle import OracleSVM
    path, m = _shipped(S, tmp_path_factory, per_class)
    assert m.form() == {"bytes": True, "class_sums": per_class == 120, "mode": 1, "msv": -1 if per_class == 120 else 5}
    osvm = OracleSVM(oracle, path)
    f = _ctx(S)
    try:
        f.load_svm_model(path, 1800)
        assert f.svm_info() == (65, m.l, 1800)
        assert f.svm_forms() == {"bytes": True, "class_sums": per_class == 120}
        z = np.load(os.path.join(GOLDEN, "svm_vectors120.npz" if per_class == 120 else "svm_vectors.npz"))
        gl, gp, gd = f.svm_predict_q8(z["q"], want_dec=True)
        _, ex = check_scores(m, osvm, z["q"], gl, gp, gd, "q8", f"golden{per_class}")
        assert (gl == z["label"]).all()
        assert np.abs(gp - z["prob"]).max() < 10 * P_TOL
        rng = np.random.default_rng(per_class)
        q = np.concatenate([E.near_vectors(rng, m.sv8.astype(np.uint8), N_MORE), rng.integers(0, 256, (29, 1800)).astype(np.uint8)])
        gl, gp, gd = f.svm_predict_q8(q, want_dec=True)
        K, ex2 = check_scores(m, osvm, q, gl, gp, gd, "q8", f"near{per_class}")
        assert (K.max(axis=1) > 0.1).mean() > 0.6
        assert_excluded(ex + ex2, len(z["q"]) + len(q), f"shipped{per_class}")
        # the double-input path on the golden vectors (all 48 kept: none of them stops within MARGIN of the threshold)
        gl, gp, gd = f.svm_predict_probability(z["q"] / 255.0, want_dec=True)
        _, ex = check_scores(m, osvm, z["q"], gl, gp, gd, "f64", f"golden{per_class}")
        assert ex == 0
    finally:
        f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("per_class", [5, 120])
def test_gpu_box_path_is_the_q8_path(S, tmp_path_factory, per_class):
    """chain_run's label and pv[label] are svm_predict_q8 of its own q rows, bit for bit: ICDAR crops, a 1080p S-text plane, random boxes (some above
    4096 px: k_ocr_hist_big), slanted boxes."""
    path, m = _shipped(S, tmp_path_factory, per_class)
    f = S.ERFilter(params=S.Params(max_width=1920, max_height=1080, max_frames=1))
    try:
        f.load_svm_model(path, 1800)
        rng = np.random.default_rng(50 + per_class)
        z = np.load(os.path.join(GOLDEN, "icdar_crops.npz"))
        planes = [S.synth.gray(z[c]) for c in sorted(z.files)] + [S.synth.gray(S.synth.stext_bgr(S.synth.frame_seed(8), 1920, 1080))]
        n_big = 0
        for pi, img in enumerate(planes):
            h, w = img.shape
            nb = 300 if pi == len(planes) - 1 else 60
            x = rng.integers(0, w - 4, nb); y = rng.integers(0, h - 4, nb)
            bw = np.minimum(rng.integers(4, 160, nb), w - x); bh = np.minimum(rng.integers(4, 120, nb), h - y)
            boxes = np.stack([x, y, bw, bh], axis=1).astype(np.int32)
            n_big += int((bw * bh > 4096).sum())
            for slope in (None, rng.uniform(-0.4, 0.4, nb)):
                q, label, prob = f.chain_run(img, boxes, slope=slope)
                gl, gp = f.svm_predict_q8(q)
                assert np.array_equal(label, gl), (pi, slope is None)
                assert np.array_equal(prob, gp[np.arange(len(q)), gl]), (pi, slope is None)
        assert n_big > 20
    finally:
        f.close()


def _pyramid_planes(oracle, frame, n_levels):
    """planes[ch][level] as the library builds them (tests/test_gpu_parity.py::test_pyramid_planes): each of Y / Cr / Cb resized level by level, an
    inverted channel 255 - its source at the same level."""
    six = oracle.compute_channels(frame)
    pyr = {c: oracle.pyramid(six[c], n_levels) for c in range(3)}
    for c in range(3):
        pyr[c + 3] = [255 - p for p in pyr[c]]
    return pyr


def _chain_per_plane(f, planes, items):
    """chain_run on each plane's boxes at once: items = [(result index, frame, ch, pyr, x, y, w, h, slope)] -> {index: (label, prob)}"""
    out = {}
    by_plane = {}
    for it in items:
        by_plane.setdefault((it[1], it[2], it[3], it[8]), []).append(it)
    for (fr, ch, pyr, slope), its in by_plane.items():
        boxes = np.array([it[4:8] for it in its], np.int32)
        _, label, prob = f.chain_run(planes[fr][ch][pyr], boxes, slope=slope)
        for it, l, p in zip(its, label, prob):
            out[it[0]] = (int(l), float(p))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("per_class", [5, 120])
def test_gpu_fused_stages_are_the_box_path(S, cascade_paths, oracle, tmp_path_factory, per_class):
    """STAGE_OCR on two frames in a two-level context: every strong / weak candidate's ocr_label / ocr_prob == chain_run on its plane's box (the fused
    path lists its candidates on the device, sizes its launches before it knows their number and reads pv[label] from the scorer); STAGE_OCR_LINES:
    every line member's line_label / line_prob == chain_run with the line's slope on its merged bound.  The planes come from the oracle's channels and
    pyramid, which equal the device's (tests/test_gpu_parity.py); chain_run is the q8 path bit for bit (test_gpu_box_path_is_the_q8_path)."""
    path, m = _shipped(S, tmp_path_factory, per_class)
    W, H = 640, 480
    frames = np.stack([S.synth.stext_bgr(S.synth.frame_seed(60 + i), W, H) for i in range(2)])
    planes = [_pyramid_planes(oracle, fr, 2) for fr in frames]
    f = S.ERFilter(params=S.Params(max_width=W, max_height=H, max_frames=2, n_pyr_levels=2))
    try:
        f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
        f.load_svm_model(path, 1800)
        res = f.text_detect(frames, S.STAGE_ALL | S.STAGE_OCR)
        c = res.cands
        on = np.flatnonzero(c["cls"] > 0)
        assert (res.ocr_label[c["cls"] == 0] == -1).all()
        assert len(on) > 20 and (c["pyr"][on] == 1).any() and (c["frame"][on] == 1).any()
        got = _chain_per_plane(f, planes, [(int(i), int(c["frame"][i]), int(c["ch"][i]), int(c["pyr"][i]), int(c["x"][i]), int(c["y"][i]),
                                            int(c["w"][i]), int(c["h"][i]), None) for i in on])
        for i in on:
            assert (int(res.ocr_label[i]), float(res.ocr_prob[i])) == got[int(i)], (int(i), c[i])
    finally:
        f.close()
    # the line stage (one pyramid level, as er_ocr runs it; the frames of test_svm.py::test_gpu_line_ocr_stage, which have slanted lines, and four more)
    F = 6
    frames = np.stack([S.synth.stext_bgr(S.synth.frame_seed(40 + i), W, H) for i in range(F)])
    planes = [_pyramid_planes(oracle, fr, 1) for fr in frames]
    g = S.ERFilter(8, 120, 900000, 2, 0.7, 0.15, max_width=W, max_height=H, max_frames=F)
    try:
        g.load_cascade(0, cascade_paths[0]); g.load_cascade(1, cascade_paths[1])
        g.load_svm_model(path, 1800)
        res = g.text_detect(frames, S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP | S.GROUP_INNER_SUP | S.STAGE_OCR_LINES)
        items, n_rot = [], 0
        for tx in res.texts:
            for j in range(int(tx["count"])):
                k = int(tx["first"]) + j
                ci = int(res.text_ers[k])
                cd, gb = res.cands[ci], res.group_bounds[ci]
                items.append((k, int(cd["frame"]), int(cd["ch"]), int(cd["pyr"]), int(gb["x"]), int(gb["y"]), int(gb["w"]), int(gb["h"]), float(tx["slope"])))
                n_rot += abs(float(tx["slope"])) > 0.01
        assert len(items) >= 4 and n_rot > 0
        got = _chain_per_plane(g, planes, items)
        for k in range(len(res.text_ers)):
            assert (int(res.line_label[k]), float(res.line_prob[k])) == got[k], k
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_q8_errors(S, tmp_path_factory):
    path, m = _shipped(S, tmp_path_factory, 5)
    f = _ctx(S)
    try:
        with pytest.raises(S.StrErError) as e:
            f.svm_predict_q8(np.zeros((1, 1800), np.uint8))
        assert e.value.code == -6                                          # STR_ER_ESTATE: no model
        f.load_svm_model(path, 1800)
        with pytest.raises(S.StrErError) as e:
            f.svm_predict_q8(np.zeros((1, 900), np.uint8))
        assert e.value.code == -1                                          # STR_ER_EINVAL: dim
        gl, gp = f.svm_predict_q8(np.zeros((0, 1800), np.uint8))
        assert gl.shape == (0,) and gp.shape == (0, 65)
    finally:
        f.close()
