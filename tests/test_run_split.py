"""str_er_feet_split and str_er_split_words on the GPU: the cuts, pieces, piece features, labels and probabilities of hand-made footprints
against the reference (run_split_ref.py: numpy profiles and tiles, the oracle's chain_features), every table with ==; the SVM half
against the q8 path bit for bit and against the exact reference (svm_exact.py) under test_svm_exact.py's comparison; the segmentation
against str_er_split_words_host and a brute force over every composition of the atoms."""
import numpy as np
import pytest

import line_words_ref as LW
import run_split_ref as RS
from test_frame_lines import _ctx
from test_line_words import _feet
from test_run_split_ref import HAND
from test_svm_exact import _shipped, assert_excluded, check_scores

pytestmark = pytest.mark.gpu
W, H = 320, 128                         # the frame of the hand-made footprints


def _profile(rng, n, h):
    """A footprint of one run with the column counts n and h rows: the pixels of a column at random rows, rows 0 and h - 1 in the
    first column that has two pixels."""
    b = np.zeros((h, len(n)), bool)
    ends = next(c for c, v in enumerate(n) if v >= 2) if h > 1 else None
    for c, v in enumerate(n):
        rows = rng.permutation(h)[:v]
        if c == ends:
            rows = np.concatenate([[0, h - 1], rng.permutation(np.arange(1, h - 1))[:v - 2]]).astype(int)
        b[rows, c] = True
    assert b.sum(axis=0).tolist() == list(n) and b[0].any() and b[h - 1].any()
    return b


def _necked(rng, h, widths, necks, lead=0):
    """A footprint whose last run is lobes of the given widths (dense, every column above h / 4) joined by necks of one pixel a
    column; lead: columns of another run and a gap in front of it."""
    cols = []
    for k, w in enumerate(widths):
        if k:
            cols += [1] * necks[k - 1]
        cols += [int(v) for v in rng.integers(h // 4 + 1, h + 1, w)]
    b = _profile(rng, cols, h) if len(cols) > 1 or h == 1 else np.ones((h, 1), bool)
    if lead:
        head = np.zeros((h, lead), bool)
        head[:, :lead - 2] = True
        b = np.concatenate([head, b], axis=1)
    return b


def _cases(rng):
    """[(name, x, y, bits, slope)] in a 320 x 128 frame: the kernel's own edges."""
    out = [(f"hand{k}", 3 + 17 * k, 2, _profile(rng, n, h), 0.0) for k, (n, h, _) in enumerate(HAND)]
    # a run that starts at foot-box column 60 whose valley lies on the columns 63 / 64: the block of the cut straddles two words
    out.append(("straddle_63", 10, 20, _necked(rng, 12, [3, 14], [2], lead=60), 0.0))
    out.append(("straddle_64", 110, 20, _necked(rng, 12, [4, 14], [2], lead=60), 0.0))
    out.append(("straddle_far", 200, 20, _necked(rng, 12, [30, 20, 9], [1, 3], lead=37), 0.0))       # both cuts past the first word of the rows
    for w in (1, 2):
        out.append((f"width_{w}", 5 + 9 * w, 40, np.ones((8, w), bool), 0.0))
    out.append(("width_64", 30, 40, _necked(rng, 8, [20, 30, 12], [1, 1]), 0.0))
    out.append(("width_65", 100, 40, _necked(rng, 8, [20, 30, 12], [2, 1]), 0.0))
    out.append(("four_ties", 170, 40, _profile(rng, [9, 2, 9, 2, 9, 2, 9, 2, 9], 12), 0.0))
    out.append(("five_ties", 185, 40, _profile(rng, [9, 1, 9, 1, 9, 1, 9, 1, 9, 1, 9], 12), 0.0))
    out.append(("five_mixed", 200, 40, _profile(rng, [9, 3, 3, 9, 2, 9, 3, 9, 2, 2, 2, 9, 1, 9], 12), 0.0))
    t = np.zeros((8, 9), bool)                                  # a piece whose row extent is tighter than its run's
    t[:, 0:3] = t[:, 7:9] = True
    t[2, 3] = t[0, 6] = True
    t[1:5, 4:6] = True
    out.append(("tight_piece", 230, 40, t, 0.0))
    a = np.zeros((30, 50), bool)                                # two lines whose footprints overlap in the frame: an open frame
    a[:, 0:3] = a[:, 47:50] = True
    a[0:3, :] = True
    out.append(("outer", 120, 90, a, 0.0))
    out.append(("inner", 125, 95, _necked(rng, 20, [12, 14, 10], [2, 2]), 0.1))          # ... and touching glyphs inside its box
    out.append(("empty", 0, 0, np.zeros((0, 0), bool), 0.0))
    out.append(("slope", 10, 60, _necked(rng, 24, [17, 21, 20], [2, 1], lead=9), 0.25))
    return out


def _many(rng, n):
    out = []
    for k in range(n):
        h, lobes = int(rng.integers(5, 20)), int(rng.integers(2, 4))
        b = _necked(rng, h, [int(rng.integers(2, 9)) for _ in range(lobes)], [int(rng.integers(1, 4)) for _ in range(lobes - 1)],
                    lead=int(rng.choice([0, 0, 6])))
        out.append((f"many{k}", int(rng.integers(0, W - b.shape[1])), int(rng.integers(0, H - h)), b, float(rng.choice([0.0, 0.0, 0.15, -0.2]))))
    return out


@pytest.fixture(scope="module")
def hand(oracle):
    """The hand-made footprints and their reference, computed once."""
    rng = np.random.default_rng(2207)
    cases = _cases(rng) + _many(rng, 70)
    feet = [(x, y, b) for _, x, y, b, _ in cases]
    slopes = [s for *_, s in cases]
    tabs, splits, pieces, line_of = RS.tables(feet)
    pq, tl = RS.piece_features(oracle, feet, pieces, line_of, slopes)
    return cases, feet, slopes, tabs, splits, pieces, line_of, pq, tl


def _check(got, tabs, splits, pieces):
    for name, a, b in zip(("line_words", "line_runs", "words"), LW.as_lists(got["line_words"], got["runs"], got["words"]), tabs):
        assert a == b, name
    gs, gp = RS.as_lists(got["splits"], got["pieces"])
    assert gs == splits
    assert gp == pieces


def test_feet_split_cuts_pieces_features(S, cascade_paths, hand):
    cases, feet, slopes, tabs, splits, pieces, line_of, pq, tl = hand
    names = [c[0] for c in cases]
    run0 = {n: tabs[0][i][2] for i, n in enumerate(names)}
    # the cases are what they claim to be
    for k, (n, h, want) in enumerate(HAND):
        s, x = splits[run0[f"hand{k}"]], 3 + 17 * k
        assert [c - x for c in s[1:1 + s[0]]] == want and s[4] == h // 4
    last = lambda name: tabs[0][names.index(name)][2] + tabs[0][names.index(name)][3] - 1
    assert splits[last("straddle_63")][:2] == (1, 10 + 63) and tabs[1][last("straddle_63")][0] == 10 + 60
    assert splits[last("straddle_64")][:2] == (1, 110 + 64) and tabs[1][last("straddle_64")][0] == 110 + 60
    assert splits[last("straddle_far")][0] == 2 and splits[last("straddle_far")][2] - 200 > 64
    assert [splits[run0[f"width_{w}"]][0] for w in (1, 2, 64, 65)] == [0, 0, 2, 2]
    assert [tabs[1][run0[f"width_{w}"]][1] - tabs[1][run0[f"width_{w}"]][0] for w in (1, 2, 64, 65)] == [1, 2, 64, 65]
    assert [c - 170 for c in splits[run0["four_ties"]][1:4]] == [1, 3, 5] and [c - 185 for c in splits[run0["five_ties"]][1:4]] == [1, 3, 5]
    assert [c - 200 for c in splits[run0["five_mixed"]][1:4]] == [4, 9, 12]
    tp = splits[run0["tight_piece"]]
    assert tp[0] == 2 and pieces[tp[5] + 2][5:7] == (41, 45) and tabs[1][run0["tight_piece"]][2:4] == (40, 48)
    # the open frame's middle is one wide valley of depth 3: the inner line's pixels inside its box do not count
    assert splits[run0["outer"]][:6] == (1, 120 + 24, -1, -1, 7, splits[run0["outer"]][5]) and splits[last("inner")][0] == 2
    assert tabs[0][names.index("empty")][3] == 0
    assert len(feet) >= 70 + 20 and sum(1 for s in splits if s[0] > 0) >= 70 and {s[0] for s in splits} == {0, 1, 2, 3}
    f = _ctx(S, cascade_paths, max_width=W, max_height=H, max_frames=1)
    try:
        ft, bits = _feet(S, feet)
        got = f.feet_split(W, H, ft, bits, slopes, want_reads=False)                 # (no model is loaded: features only)
        assert got["reads"] is None and got["piece_reads"] is None
        _check(got, tabs, splits, pieces)
        assert got["piece_q"].shape == pq.shape
        bad = np.flatnonzero((got["piece_q"] != pq).any(axis=1))
        assert len(bad) == 0, [(int(i), pieces[i]) for i in bad[:8]]
        # the runs' own results are those of feet_read
        *_, rq = f.feet_read(W, H, ft, bits, slopes, want_reads=False)
        assert got["q"].tobytes() == rq.tobytes()
        # cuts and pieces alone; the same bytes again
        lean = f.feet_split(W, H, ft, bits, slopes, want_reads=False, want_q=False)
        assert lean["piece_q"] is None
        _check(lean, tabs, splits, pieces)
        again = f.feet_split(W, H, ft, bits, slopes, want_reads=False)
        for k in ("splits", "pieces", "piece_q", "q", "runs"):
            assert again[k].tobytes() == got[k].tobytes(), k
        # each of the first cases alone (another grid, another atlas)
        for i in range(len(feet) - 70):
            one = f.feet_split(W, H, *_feet(S, [feet[i]]), [slopes[i]], want_reads=False)
            lo, n = tabs[0][i][2], tabs[0][i][3]
            s1, p1 = RS.as_lists(one["splits"], one["pieces"])
            fp = splits[lo][5] if n else 0
            want_s = [(*s[:5], s[5] - fp, *s[6:]) for s in splits[lo:lo + n]]
            want_p = [(p[0] - lo, *p[1:]) for p in pieces if lo <= p[0] < lo + n]
            assert s1 == want_s and p1 == want_p, names[i]
            assert (one["piece_q"] == pq[fp:fp + len(want_p)]).all(), names[i]
        # thresholds that cut nowhere
        for num, den in ((1, 65535), (65535, 65535)):
            f.set_run_split(num, den)
            none = f.feet_split(W, H, ft, bits, slopes, want_reads=False)
            want_thr = [RS.threshold(r[3] - r[2], num, den) for r in tabs[1]]
            assert (none["splits"]["n_cuts"] == 0).all() and len(none["pieces"]) == 0 and none["splits"]["thr"].tolist() == want_thr
            assert none["piece_q"].shape == (0, 1800) and none["q"].tobytes() == rq.tobytes()
        # another threshold: 1 / 2
        f.set_run_split(1, 2)
        half = RS.tables(feet, 1, 2)
        _check(f.feet_split(W, H, ft, bits, slopes, want_reads=False, want_q=False), *half[:3])
        assert half[1] != splits
        f.set_run_split()
        # labels need a model; the context works afterwards
        with pytest.raises(S.StrErError) as e:
            f.feet_split(W, H, ft, bits, slopes)
        assert e.value.code == -6 and "str_er_feet_split" in str(e.value) and "1800" in str(e.value)
        _check(f.feet_split(W, H, ft, bits, slopes, want_reads=False, want_q=False), tabs, splits, pieces)
        # nothing at all
        z = f.feet_split(W, H, *_feet(S, []), None, want_reads=False)
        assert len(z["runs"]) == len(z["splits"]) == len(z["pieces"]) == len(z["piece_q"]) == 0
    finally:
        f.close()


def test_feet_split_wide_runs(S, cascade_paths):
    """Runs of 1024 and 1025 columns, 8 rows: the widest run that is split and the first that is not."""
    rng = np.random.default_rng(5)
    FW, FH = 2200, 64
    lobes = lambda total: [total - 3 - 700 - 200, 700, 200]
    a, b = _necked(rng, 8, lobes(1024), [1, 2]), _necked(rng, 8, lobes(1025), [1, 2], lead=70)
    assert a.shape == (8, 1024) and b.shape == (8, 1025 + 70)
    feet = [(100, 0, a), (1000, 8, b)]
    tabs, splits, pieces, line_of = RS.tables(feet)
    assert [r[1] - r[0] for r in tabs[1]] == [1024, 68, 1025] and [s[0] for s in splits] == [2, 0, 0] and len(pieces) == 5
    assert splits[0][1:3] == (100 + 121, 100 + 121 + 1 + 700) and splits[2][4] == 2
    f = _ctx(S, cascade_paths, max_width=FW, max_height=FH, max_frames=1)
    try:
        got = f.feet_split(FW, FH, *_feet(S, feet), None, want_reads=False, want_q=False)
        _check(got, tabs, splits, pieces)
    finally:
        f.close()


def test_feet_split_labels(S, cascade_paths, oracle, tmp_path_factory, hand):
    from oracle.oracle import OracleSVM
    cases, feet, slopes, tabs, splits, pieces, line_of, pq, tl = hand
    path, m = _shipped(S, tmp_path_factory, 5)
    f = _ctx(S, cascade_paths, max_width=W, max_height=H, max_frames=1)
    try:
        f.load_svm_model(path, 1800)
        ft, bits = _feet(S, feet)
        got = f.feet_split(W, H, ft, bits, slopes)
        _check(got, tabs, splits, pieces)
        assert (got["piece_q"] == pq).all() and len(got["piece_reads"]) == len(pq)
        # the runs' own reads are those of feet_read, byte for byte
        _, _, _, reads, rq = f.feet_read(W, H, ft, bits, slopes)
        assert got["reads"].tobytes() == reads.tobytes() and got["q"].tobytes() == rq.tobytes()
        # label and prob are svm_predict_q8 of the reference's feature rows, bit for bit
        pr = got["piece_reads"]
        gl, gp, gd = f.svm_predict_q8(pq, want_dec=True)
        assert np.array_equal(pr["label"], gl)
        assert np.array_equal(pr["prob"], gp[np.arange(len(pq)), gl])
        # ... and the q8 path agrees with the exact reference under test_svm_exact.py's comparison
        _, ex = check_scores(m, OracleSVM(oracle, path), pq, gl, gp, gd, "q8", "run_split")
        assert_excluded(ex, len(pq), "run_split")
        assert [chr(int(c)) for c in pr["ch"]] == [S.ocr_char(int(l)) for l in pr["label"]]
    finally:
        f.close()


# ---- str_er_split_words ------------------------------------------------------------------------------------------------------------------

def _random_rows(S, rng, n_runs, hi, cuts=None):
    """Random split records and cost rows: n_cuts 0 .. 3 (or `cuts`), the piece rows back to back."""
    sp = np.zeros(n_runs, S.RUN_SPLIT_DTYPE)
    sp["cut"] = -1
    sp["n_cuts"] = rng.integers(0, 4, n_runs) if cuts is None else cuts
    sp["n_pieces"] = [len(RS.piece_nodes(int(k) + 1)) for k in sp["n_cuts"]]
    sp["first_piece"] = np.concatenate([[0], np.cumsum(sp["n_pieces"])[:-1]]) if n_runs else []
    n_pc = int(sp["n_pieces"].sum())
    return sp, rng.integers(0, hi, (n_runs, 65)).astype(np.uint8), rng.integers(0, hi, (n_pc, 65)).astype(np.uint8)


def _as_ref(sp):
    return [(int(s["n_cuts"]), *[int(v) for v in s["cut"]], int(s["thr"]), int(s["first_piece"]), int(s["n_pieces"]), 0) for s in sp]


def _same_split(S, f, sp, rc, pc, first, n_of, split):
    f.set_run_split(1, 4, split)
    gw, gp, gr = f.split_words(sp, rc, pc, first, n_of)
    hw, hp, hr = S.split_words_host(sp, rc, pc, first, n_of, split)
    assert gw.tobytes() == hw.tobytes() and gp.tobytes() == hp.tobytes() and gr.tobytes() == hr.tobytes()
    bw, bp, br = RS.split_words(_as_ref(sp), rc, pc, first, n_of, split)
    assert [tuple(int(v) for v in w) for w in gw.tolist()] == bw
    assert [tuple(int(v) for v in p) for p in gp.tolist()] == bp
    assert gr.shape == br.shape and (gr == br).all()
    assert (gw["cost"] <= gw["read_cost"]).all() and (gw["n_parts"] >= np.asarray(n_of)).all()
    return gw, gp, gr


def test_split_words_equals_host_and_brute_force(S, cascade_paths):
    rng = np.random.default_rng(41)
    f = _ctx(S, cascade_paths, max_width=W, max_height=H, max_frames=1)
    try:
        # 1000 words over 2400 runs, windows that overlap and words of 0 runs; small ranges tie often
        for hi, split in ((256, 8), (256, 0), (4, 0), (16, 255), (2, 8)):
            sp, rc, pc = _random_rows(S, rng, 2400, hi)
            first = rng.integers(0, 2400 - 6, 1000)
            n_of = rng.integers(0, 7, 1000)
            n_of[::97] = 0
            gw, gp, gr = _same_split(S, f, sp, rc, pc, first, n_of, split)
            assert (gw["n_parts"][::97] == 0).all() and (gw["cost"][::97] == 0).all()
            if hi == 256:
                assert (gw["n_parts"] > n_of).any() and (gw["cost"] < gw["read_cost"]).any()
            if split == 255 and hi == 16:
                assert (gw["n_parts"] == n_of).all() and (gw["cost"] == gw["read_cost"]).all() and (gp["piece"] == -1).all()
        # every n_cuts alone; rows all 255: the run stays whole at any SPLIT
        for k in range(4):
            sp, rc, pc = _random_rows(S, rng, 50, 256, cuts=k)
            _same_split(S, f, sp, rc, pc, np.arange(50), np.ones(50, int), 8)
            rc[:], pc[:] = 255, 255
            gw, gp, _ = _same_split(S, f, sp, rc, pc, np.arange(50), np.ones(50, int), 8)
            assert (gw["n_parts"] == 1).all() and (gw["cost"] == 255).all()
            gw, gp, _ = _same_split(S, f, sp, rc, pc, np.arange(50), np.ones(50, int), 0)
            assert (gw["n_parts"] == 1).all() and (gp["piece"] == -1).all()
        # a word of 33 parts and more: 11 runs of 4 atoms whose pieces are free
        sp, rc, pc = _random_rows(S, rng, 11, 256, cuts=3)
        rc[:] = 200
        pc[:] = 200
        for s in sp:
            for i in (0, 3, 6, 8):                              # the atoms (0, 1), (1, 2), (2, 3), (3, 4)
                pc[int(s["first_piece"]) + i, 3] = 0
        gw, gp, gr = _same_split(S, f, sp, rc, pc, [0, 0, 2], [11, 8, 9], 8)
        assert gw["n_parts"].tolist() == [44, 32, 36] and gw["first_part"].tolist() == [0, 44, 76] and gw["cost"].tolist() == [11 * 24, 8 * 24, 9 * 24]
        assert RS.split_text(gp[:44], gr[:44]) == ["3"] * 44
        sp, rc, pc = _random_rows(S, rng, 33, 256, cuts=0)
        gw, gp, gr = _same_split(S, f, sp, rc, pc, [0], [33], 8)
        assert gw["n_parts"].tolist() == [33] and (gr == rc).all()
        # nothing at all
        gw, gp, gr = f.split_words(sp[:0], rc[:0], pc[:0], [], [])
        assert len(gw) == len(gp) == len(gr) == 0
        gw, gp, gr = f.split_words(sp[:0], rc[:0], pc[:0], [0, 0], [0, 0])
        assert gw.tolist() == [(0, 0, 0, 0)] * 2 and len(gp) == 0
    finally:
        f.close()
