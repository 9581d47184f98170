"""STR_ER_WANT_RUN_READ / str_er_feet_read on the GPU: the tile, features, label, probability and character of every glyph run against
the reference (run_read_ref.py: numpy tiles, the oracle's chain_features), every byte with ==; the SVM half against the q8 path bit for
bit and against the exact reference (svm_exact.py) under test_svm_exact.py's comparison."""
import numpy as np
import pytest

import line_words_ref as LW
import run_read_ref as RR
import svm_exact as E
from test_frame_lines import GROUPED, _ctx, _same, reference as frame_lines_reference
from test_line_words import _feet
from test_svm_exact import _shipped, assert_excluded, check_scores

pytestmark = pytest.mark.gpu
W, H = 320, 128                         # the frame of the hand-made footprints
TABLES = ("line_words", "line_runs", "words")


def _glyphs(rng, w, h, spans, p=0.55):
    """A tight footprint of w x h whose runs are the column spans [(c0, c1), ...]: random pixels, every column of a span with one,
    the first and the last row with one."""
    b = np.zeros((h, w), bool)
    for c0, c1 in spans:
        b[:, c0:c1] = rng.random((h, c1 - c0)) < p
        for c in range(c0, c1):
            if not b[:, c].any():
                b[rng.integers(0, h), c] = True
    c = spans[0][0]
    b[0, c] = b[h - 1, c] = True
    assert b[:, 0].any() and b[:, w - 1].any()
    return b


def _cases(rng):
    """[(name, x, y, bits, slope)]: every shape the issue names, in a 320 x 128 frame."""
    out = []
    # runs that straddle columns 60-70 and 120-135 of the foot box: they cross the 64-column words of the footprint rows
    out.append(("straddles", 5, 3, _glyphs(rng, 150, 21, [(0, 9), (57, 73), (80, 82), (118, 137), (141, 150)]), 0.0))
    out.append(("width_64", 17, 40, _glyphs(rng, 64, 13, [(0, 20), (22, 61), (63, 64)]), 0.0))
    out.append(("width_65", 200, 50, _glyphs(rng, 65, 13, [(0, 30), (33, 63), (64, 65)]), 0.0))
    out.append(("one_run_of_64", 100, 70, _glyphs(rng, 64, 9, [(0, 64)]), 0.0))
    out.append(("one_run_of_65", 101, 71, _glyphs(rng, 65, 9, [(0, 65)]), 0.0))
    out.append(("one_column", 31, 90, _glyphs(rng, 1, 17, [(0, 1)]), 0.0))
    out.append(("one_pixel", 319, 127, np.ones((1, 1), bool), 0.0))
    solid = np.zeros((20, 40), bool)
    solid[:, 0:12] = True                                      # a solid run: its tile is all 0
    solid[3:15, 20:40] = _glyphs(rng, 20, 12, [(0, 20)])
    out.append(("solid", 60, 100, solid, 0.0))
    out.append(("big_72x64", 240, 60, _glyphs(rng, 72, 64, [(0, 72)], 0.5), 0.0))          # 4608 pixels: the scorer's other histogram path
    out.append(("slope_up", 10, 60, _glyphs(rng, 90, 24, [(0, 17), (20, 41), (45, 66), (70, 90)]), 0.25))
    out.append(("slope_down", 150, 5, _glyphs(rng, 90, 24, [(0, 23), (25, 44), (50, 90)]), -0.4))
    out.append(("empty", 0, 0, np.zeros((0, 0), bool), 0.0))
    a = np.zeros((30, 50), bool)                               # two lines whose footprints overlap in the frame: an open frame
    a[:, 0:3] = a[:, 47:50] = True
    a[0:3, :] = True
    out.append(("outer", 120, 90, a, 0.0))
    out.append(("inner", 125, 95, _glyphs(rng, 40, 20, [(0, 18), (22, 40)]), 0.1))         # ... and glyphs inside its box
    return out


def _many(rng, n):
    out = []
    for k in range(n):
        w, h = int(rng.integers(6, 40)), int(rng.integers(5, 20))
        cut = int(rng.integers(2, w - 2))
        out.append((f"many{k}", int(rng.integers(0, W - w)), int(rng.integers(0, H - h)), _glyphs(rng, w, h, [(0, cut), (cut + 1, w)]),
                    float(rng.choice([0.0, 0.0, 0.15, -0.2]))))
    return out


@pytest.fixture(scope="module")
def hand(oracle):
    """The hand-made footprints and their reference, computed once: (cases, feet, slopes, tables, features, tiles)."""
    rng = np.random.default_rng(2118)
    cases = _cases(rng) + _many(rng, 70)
    feet = [(x, y, b) for _, x, y, b, _ in cases]
    slopes = [s for *_, s in cases]
    tabs, q, tl = RR.features(oracle, feet, slopes)
    return cases, feet, slopes, tabs, q, tl


def _check_tables(got, tabs):
    for name, a, b in zip(TABLES, LW.as_lists(*got), tabs):
        assert a == b, name


# ---- 1. str_er_feet_read on hand-made footprints: the features ---------------------------------------------------------------------------

def test_feet_read_features(S, cascade_paths, hand):
    cases, feet, slopes, tabs, q, tl = hand
    names = [c[0] for c in cases]
    # the cases are what they claim to be
    runs_of = {n: tabs[1][tabs[0][i][2]:tabs[0][i][2] + tabs[0][i][3]] for i, n in enumerate(names)}
    x = 5
    assert [(r[0] - x, r[1] - x) for r in runs_of["straddles"]] == [(0, 9), (57, 73), (80, 82), (118, 137), (141, 150)]
    assert len(runs_of["empty"]) == 0 and runs_of["one_pixel"] == [(319, 320, 127, 128, 1, runs_of["one_pixel"][0][5])]
    assert runs_of["one_column"][0][1] - runs_of["one_column"][0][0] == 1
    big = runs_of["big_72x64"][0]
    assert (big[1] - big[0]) * (big[3] - big[2]) == 72 * 64 > 4096
    first = tabs[0][names.index("solid")][2]
    assert (tl[first] == 0).all() and tl[first].shape == (20, 12)
    outer = tabs[0][names.index("outer")][2]
    assert tl[outer].shape == (30, 50) and (tl[outer][5:25, 5:45] == 255).all()            # the inner line's pixels are not the outer's
    assert len(feet) >= 70 + 14 and len(q) > 150
    f = _ctx(S, cascade_paths, max_width=W, max_height=H, max_frames=1)
    try:
        ft, bits = _feet(S, feet)
        lw, runs, words, reads, gq = f.feet_read(W, H, ft, bits, slopes, want_reads=False)                 # (no model is loaded: features only)
        assert reads is None
        _check_tables((lw, runs, words), tabs)
        assert gq.shape == q.shape
        bad = np.flatnonzero((gq != q).any(axis=1))
        assert len(bad) == 0, [(int(i), tabs[1][i]) for i in bad[:8]]
        # without slopes: all 0
        flat = [i for i, s in enumerate(slopes) if s == 0.0]
        *_, gq0 = f.feet_read(W, H, ft, bits, None, want_reads=False)
        line_of = np.concatenate([np.full(l[3], t) for t, l in enumerate(tabs[0])])
        assert (gq0[np.isin(line_of, flat)] == q[np.isin(line_of, flat)]).all()
        assert (gq0[~np.isin(line_of, flat)] != q[~np.isin(line_of, flat)]).any()
        # each of the first cases alone (another atlas, another grid)
        for i in range(len(feet) - 70):
            ft1, b1 = _feet(S, [feet[i]])
            _, r1, _, _, q1 = f.feet_read(W, H, ft1, b1, [slopes[i]], want_reads=False)
            lo = tabs[0][i][2]
            assert len(r1) == tabs[0][i][3] and (q1 == q[lo:lo + len(r1)]).all(), names[i]
        # reads need a model; a slope that is not a number is refused; the context works afterwards
        with pytest.raises(S.StrErError) as e:
            f.feet_read(W, H, ft, bits, slopes)
        assert e.value.code == -6 and "1800" in str(e.value)
        badsl = list(slopes)
        badsl[3] = float("nan")
        with pytest.raises(S.StrErError) as e:
            f.feet_read(W, H, ft, bits, badsl, want_reads=False)
        assert e.value.code == -1
        badsl[3] = float("inf")
        with pytest.raises(S.StrErError) as e:
            f.feet_read(W, H, ft, bits, badsl, want_reads=False)
        assert e.value.code == -1
        *_, again = f.feet_read(W, H, ft, bits, slopes, want_reads=False)
        assert (again == q).all()
        # nothing at all
        lw, runs, words, reads, gq = f.feet_read(W, H, *_feet(S, []), None, want_reads=False)
        assert len(lw) == len(runs) == len(words) == len(gq) == 0
    finally:
        f.close()


# ---- 2. the same input with the fixture model ------------------------------------------------------------------------------------------

def test_feet_read_labels(S, cascade_paths, oracle, tmp_path_factory, hand):
    from oracle.oracle import OracleSVM
    cases, feet, slopes, tabs, q, tl = hand
    path, m = _shipped(S, tmp_path_factory, 5)
    f = _ctx(S, cascade_paths, max_width=W, max_height=H, max_frames=1)
    try:
        f.load_svm_model(path, 1800)
        ft, bits = _feet(S, feet)
        lw, runs, words, reads, gq = f.feet_read(W, H, ft, bits, slopes)
        _check_tables((lw, runs, words), tabs)
        assert (gq == q).all() and len(reads) == len(q)
        # label and prob are svm_predict_q8 of the reference's feature rows, bit for bit
        gl, gp, gd = f.svm_predict_q8(q, want_dec=True)
        assert np.array_equal(reads["label"], gl)
        assert np.array_equal(reads["prob"], gp[np.arange(len(q)), gl])
        # ... and the q8 path agrees with the exact reference under test_svm_exact.py's comparison
        _, ex = check_scores(m, OracleSVM(oracle, path), q, gl, gp, gd, "q8", "run_read")
        assert_excluded(ex, len(q), "run_read")
        assert [int(c) for c in reads["ch"]] == [ord(RR.ocr_char(int(l))) for l in reads["label"]]
        assert [chr(int(c)) for c in reads["ch"]] == [S.ocr_char(int(l)) for l in reads["label"]]
    finally:
        f.close()


# ---- 3. the detect call ----------------------------------------------------------------------------------------------------------------

def _check_detect(S, oracle, res, sizes):
    """Every run's reading of a result that carries its masks against the reference; returns the number of lines with two or more words."""
    ft = frame_lines_reference(res, sizes)[0]
    feet = [(g.x, g.y, g.bits) for g in ft]
    slopes = [float(t["slope"]) for t in res.texts]
    tabs, q, _ = RR.features(oracle, feet, slopes)
    _check_tables((res.line_words, res.line_runs, res.words), tabs)
    assert res.run_features.shape == q.shape and (res.run_features == q).all()
    assert len(res.run_reads) == len(res.line_runs)
    chars = [chr(int(c)) for c in res.run_reads["ch"]]
    assert chars == [RR.ocr_char(int(l)) for l in res.run_reads["label"]]
    strings = RR.word_strings(tabs, chars)
    assert [res.word_text(w) for w in range(len(res.words))] == strings
    for t, lw in enumerate(tabs[0]):
        assert res.words_text_of_line(t) == strings[lw[0]:lw[0] + lw[1]]
    for i, g in enumerate(res.frame_lines):
        assert res.frame_line_text(i) == " ".join(res.words_text_of_line(int(g["rep"])))
    return sum(1 for lw in tabs[0] if lw[1] >= 2)


def _same_reads(a, b):
    for k in TABLES + ("run_reads", "run_features"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def test_detect_reads_every_run(S, cascade_paths, oracle, tmp_path_factory):
    path, m = _shipped(S, tmp_path_factory, 5)
    prm = S.Params(max_width=640, max_height=480, max_frames=2, n_pyr_levels=2)
    f = S.ERFilter(params=prm)
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    f.load_svm_model(path, 1800)
    sy = S.synth
    uniform = np.stack([sy.stext_bgr(sy.frame_seed(2), 640, 480), sy.stext_bgr(sy.frame_seed(976), 640, 480)])
    ragged = [uniform[0], sy.stext_bgr(sy.frame_seed(971), 333, 211)]
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS
    try:
        res = f.text_detect(uniform, GROUPED, want_masks=True, want_frame_lines=True, want_line_words=True, want_run_read=True)
        two = _check_detect(S, oracle, res, [(640, 480)] * 2)
        assert two >= 1 and {int(t["frame"]) for t in res.texts} == {0, 1}
        # label and prob are the q8 path of the features
        gl, gp = f.svm_predict_q8(res.run_features)
        assert np.array_equal(res.run_reads["label"], gl) and np.array_equal(res.run_reads["prob"], gp[np.arange(len(gl)), gl])
        # every other table is that of the call without the flag
        plain = f.text_detect(uniform, GROUPED, want_masks=True, want_frame_lines=True, want_line_words=True)
        with pytest.raises(ValueError):
            plain.run_reads
        _same(plain, res)
        for k in TABLES + ("line_feet", "line_pairs", "frame_lines", "frame_line_members", "masks", "mask_bits"):
            assert getattr(plain, k).tobytes() == getattr(res, k).tobytes(), k
        lst = f.text_detect_list(ragged, GROUPED, want_masks=True, want_frame_lines=True, want_line_words=True, want_run_read=True)
        assert _check_detect(S, oracle, lst, [(640, 480), (333, 211)]) >= 1 and {int(t["frame"]) for t in lst.texts} == {0, 1}
        lean = f.text_detect_list(ragged, flags | S.WANT_RUN_READ)          # (without the masks in the result: the stage makes them)
        _same_reads(lean, lst)
        # the same submissions through a stream, record for record
        st = S.FrameStream(prm, depth=2)
        st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
        st.load_svm_model(path, 1800)
        try:
            st.submit_copy(uniform, flags | S.WANT_MASKS, want_run_read=True)
            st.submit_copy_list(ragged, flags, want_run_read=True)
            _, a = st.next()                                       # (two staging buffers: one result is collected before the third submission)
            _same_reads(a, res)
            st.submit_copy_list(ragged, flags)
            _, b = st.next()
            _same_reads(b, lst)
            _, c = st.next()
            with pytest.raises(ValueError):
                c.run_reads
            assert c.line_runs.tobytes() == lst.line_runs.tobytes()
        finally:
            st.close()
        # a grouped call without lines: empty tables, not an error
        blank = f.text_detect(np.full((120, 160, 3), 128, np.uint8), flags | S.WANT_RUN_READ)
        assert len(blank.texts) == 0 and len(blank.run_reads) == 0 and blank.run_features.shape == (0, 1800)
    finally:
        f.close()


# ---- 4. errors -------------------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_context_usable(S, cascade_paths, tmp_path_factory):
    path, m = _shipped(S, tmp_path_factory, 5)
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=1)
    frame = S.synth.stext_bgr(S.synth.frame_seed(2), 640, 480)         # (the frame of test_line_words.py: it has lines with runs)
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS
    try:
        ws = f.workspace_bytes()
        with pytest.raises(S.StrErError) as e:                           # without a model
            f.text_detect(frame, flags | S.WANT_RUN_READ)
        assert e.value.code == -6 and "STR_ER_WANT_RUN_READ" in str(e.value)
        assert f.run_atlas_stats() == (0, 0) and f.workspace_bytes() == ws
        f.load_svm_model(path, 1800)
        ws = f.workspace_bytes()
        with pytest.raises(S.StrErError) as e:                           # without STR_ER_WANT_LINE_WORDS
            f.text_detect(frame, GROUPED | S.WANT_FRAME_LINES | S.WANT_RUN_READ)
        assert e.value.code == -1 and "STR_ER_WANT_RUN_READ" in str(e.value)
        with pytest.raises(S.StrErError) as e:
            f.text_detect(frame, GROUPED | S.WANT_RUN_READ)
        assert e.value.code == -1 and "STR_ER_WANT_RUN_READ" in str(e.value)
        planes = f.compute_channels(frame)                               # the per-plane calls
        with pytest.raises(S.StrErError) as e:
            f.detect_planes(planes[:1], S.STAGE_ALL | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS | S.WANT_RUN_READ)
        assert e.value.code == -1 and "STR_ER_WANT_RUN_READ" in str(e.value)
        assert f.run_atlas_stats() == (0, 0) and f.workspace_bytes() == ws
        plain = f.text_detect(frame, flags)                               # a call without the flag makes no atlas
        assert f.run_atlas_stats() == (0, 0) and len(plain.line_runs) > 0
        good = f.text_detect(frame, flags | S.WANT_RUN_READ)
        assert len(good.run_reads) == len(good.line_runs) == len(plain.line_runs) and f.run_atlas_stats()[1] == 1
        assert f.workspace_bytes() == ws
    finally:
        f.close()


# ---- 5. few, many, few runs on one context ---------------------------------------------------------------------------------------------

def test_atlas_grows_once(S, cascade_paths, hand):
    cases, feet, slopes, tabs, q, tl = hand
    f = _ctx(S, cascade_paths, max_width=W, max_height=H, max_frames=1)
    try:
        few = [1, 2]                                       # width_64 and width_65: small tiles
        lo, hi = tabs[0][few[0]][2], tabs[0][few[-1]][2] + tabs[0][few[-1]][3]
        ft1, b1 = _feet(S, [feet[i] for i in few])
        ft, bits = _feet(S, feet)
        *_, q1 = f.feet_read(W, H, ft1, b1, [slopes[i] for i in few], want_reads=False)
        size1, grown1 = f.run_atlas_stats()
        assert (q1 == q[lo:hi]).all() and grown1 == 1 and size1 > 0
        *_, q2 = f.feet_read(W, H, ft, bits, slopes, want_reads=False)
        size2, grown2 = f.run_atlas_stats()
        assert (q2 == q).all() and grown2 == 2 and size2 > size1
        *_, q3 = f.feet_read(W, H, ft1, b1, [slopes[i] for i in few], want_reads=False)
        assert (q3 == q1).all() and f.run_atlas_stats() == (size2, 2)
        *_, q4 = f.feet_read(W, H, ft, bits, slopes, want_reads=False)
        assert (q4 == q).all() and f.run_atlas_stats() == (size2, 2)
    finally:
        f.close()
