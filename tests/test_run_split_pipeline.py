"""STR_ER_WANT_RUN_SPLIT in the detect calls: every new table against the reference (run_split_ref.py) built from the same result's
footprints (want_masks) and against str_er_split_words_host on the returned rows; the matcher's and the decoder's tables are
match_words / decode_words on the parts' rows; every table of a call without the flag is byte for byte what it was, and so are the
runs' own reads within the flagged call; the same through a list call and a stream submission.

Which frames give the cuts (fixed on the GPU, where the footprints are made): the list call holds the four shipped ICDAR crops
(golden/icdar_crops.npz) and the S-text frame of seed 971 (333 x 211); the frame call the S-text frames of seeds 2 and 976.  Under the
shipped cascades the four crops give no text line at two pyramid levels (0 lines; 1 line with three levels or a finer threshold
step, with no cut run at 1 / 4 .. 9 / 10), so the cut runs are those of the S-text frames, whose footprints are unions of glyph
boxes: at NUM / DEN = 1 / 2 the list call has 10 runs of which 7 are cut (17 pieces), the frame call 29 runs of which 22 are cut
(101 pieces); at the default 1 / 4: 4 and 23.  test_detect_splits_every_run asserts the 5 cut runs the condition asks for.

The second condition -- a word with n_parts > n_runs -- cannot be met with a shipped model: with either the class probabilities of
these tiles are near 1 / 65 (the cheapest character of a row costs 45 .. 47 with 5 samples a class, 39 .. 44 with 120, in 1/8 bit),
so two pieces (>= 78) never cost less than the whole run (<= 47) at any SPLIT >= 0: measured 0 words of 9, 22, 12 and 12 on four
frame sets at 1 / 4, 1 / 2, 2 / 3 and 9 / 10 with SPLIT 0, 2 and 8.  test_a_detected_word_splits therefore loads a model of the test's
own (run_split_ref.prototype_model: one support vector a class, the feature rows of pieces of the frame call, atoms first), which
reads those pieces with a high probability and everything else at 1 / 65; with it words split in the detect calls, the condition is
asserted, and the matcher and the decoder are held on split sequences that differ from the runs."""
import numpy as np
import pytest

import run_split_ref as RS
import word_match_ref as WM
from test_frame_lines import GROUPED, _crops, _same, reference as frame_lines_reference
from test_svm_exact import _shipped
from test_word_match_pipeline import TABLES, WANTS

pytestmark = pytest.mark.gpu
NUM, DEN, SPLIT = 1, 2, 8
SPLIT_TABLES = ("run_splits", "run_pieces", "piece_reads", "piece_costs", "split_parts", "word_splits", "run_costs")


@pytest.fixture(scope="module")
def scene(S, cascade_paths, tmp_path_factory):
    path, m = _shipped(S, tmp_path_factory, 5)
    prm = S.Params(max_width=640, max_height=480, max_frames=5, n_pyr_levels=2)
    f = S.ERFilter(params=prm)
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    f.load_svm_model(path, 1800)
    sy = S.synth
    uniform = np.stack([sy.stext_bgr(sy.frame_seed(2), 640, 480), sy.stext_bgr(sy.frame_seed(976), 640, 480)])
    crops = _crops() + [sy.stext_bgr(sy.frame_seed(971), 333, 211)]
    empty = f.run_split_stats()
    plain = f.text_detect(uniform, GROUPED, **WANTS)
    plain_crops = f.text_detect_list(crops, GROUPED, **WANTS)
    assert f.run_split_stats() == empty == (0, 0)                        # a call without the flag makes none of the flag's buffers
    f.set_run_split(NUM, DEN, SPLIT)
    yield S, f, prm, path, np.asarray(m.label, np.int64), uniform, crops, plain, plain_crops
    f.close()


def _part_rows(res):
    """The cost rows of the parts of a result, in part order."""
    return np.array([res.run_costs[int(p["run"])] if int(p["piece"]) < 0 else res.piece_costs[int(p["piece"])] for p in res.split_parts],
                    np.uint8).reshape(-1, 65)


def check_split(S, f, oracle, res, sizes, labels, fold=False):
    """Every table of the flag against the reference; returns (cut runs, words with more parts than runs)."""
    print(f"{len(res.texts)} lines, {len(res.line_runs)} runs, {int((res.run_splits['n_cuts'] > 0).sum())} cut, {len(res.run_pieces)} pieces, {len(res.words)} words, "
          f"{int((res.word_splits['n_parts'] > res.words['n_runs']).sum())} with more parts than runs")
    ft = frame_lines_reference(res, sizes)[0]
    feet = [(g.x, g.y, g.bits) for g in ft]
    slopes = [float(t["slope"]) for t in res.texts]
    tabs, splits, pieces, line_of = RS.tables(feet, NUM, DEN)
    gs, gp = RS.as_lists(res.run_splits, res.run_pieces)
    assert [s[:7] for s in gs] == [s[:7] for s in splits] and gp == pieces
    n, n_pc = len(res.line_runs), len(pieces)
    assert len(res.run_splits) == n and res.piece_costs.shape == (n_pc, 65) and len(res.piece_reads) == n_pc and len(res.word_splits) == len(res.words)
    # the pieces' reads: the q8 path of the reference's features, their rows the costs of its probabilities
    pq, _ = RS.piece_features(oracle, feet, pieces, line_of, slopes)
    if n_pc:
        gl, gpr = f.svm_predict_q8(pq)
        assert np.array_equal(res.piece_reads["label"], gl) and np.array_equal(res.piece_reads["prob"], gpr[np.arange(n_pc), gl])
        assert (res.piece_costs == S.prob_costs(gpr, labels, fold)).all() and (res.piece_costs == WM.cost_rows(gpr, labels, fold)).all()
    assert res.run_costs.shape == (n, 65)
    # the segmentation: the host's rules and the brute force on the returned rows
    first, n_of = res.words["first_run"], res.words["n_runs"]
    hw, hp, hr = S.split_words_host(res.run_splits, res.run_costs, res.piece_costs, first, n_of, SPLIT)
    assert hw.tobytes() == res.word_splits.tobytes() and hp.tobytes() == res.split_parts.tobytes()
    bw, bp, br = RS.split_words(splits, res.run_costs, res.piece_costs, first, n_of, SPLIT)
    assert [tuple(int(v) for v in w) for w in res.word_splits.tolist()] == bw and [tuple(int(v) for v in p) for p in res.split_parts.tolist()] == bp
    gw, gpt, gr = f.split_words(res.run_splits, res.run_costs, res.piece_costs, first, n_of)
    assert gw.tobytes() == hw.tobytes() and gpt.tobytes() == hp.tobytes() and gr.tobytes() == hr.tobytes()
    assert (hr == _part_rows(res)).all()
    assert res.run_splits["n_parts"].tolist() == np.bincount(res.split_parts["run"], minlength=n).tolist()
    ws = res.word_splits
    assert (ws["cost"] <= ws["read_cost"]).all() and (ws["n_parts"] >= n_of).all()
    assert ws["read_cost"].tolist() == [int(res.run_costs[a:a + k].min(axis=1).astype(np.int64).sum()) for a, k in zip(first, n_of)]
    # the texts
    chars = RS.split_text(res.split_parts, hr)
    for w in range(len(res.words)):
        a, k = int(ws[w]["first_part"]), int(ws[w]["n_parts"])
        assert res.word_split_text(w) == "".join(chars[a:a + k])
    for t in range(len(res.line_words)):
        lw = res.line_words[t]
        assert res.words_split_text_of_line(t) == [res.word_split_text(w) for w in range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))]
    for i, g in enumerate(res.frame_lines):
        assert res.frame_line_split_text(i) == " ".join(res.words_split_text_of_line(int(g["rep"])))
    return int((res.run_splits["n_cuts"] > 0).sum()), int((ws["n_parts"] > n_of).sum())


def test_detect_splits_every_run(scene, oracle):
    S, f, prm, path, labels, uniform, crops, plain, plain_crops = scene
    sizes = [(c.shape[1], c.shape[0]) for c in crops]
    res = f.text_detect_list(crops, GROUPED, want_run_split=True, **WANTS)
    cut, longer = check_split(S, f, oracle, res, sizes, labels)
    assert cut >= 5
    # every other table is that of the call without the flag, and the runs' own reads are what they were
    for name in ("run_splits", "run_pieces", "piece_reads", "piece_costs", "split_parts", "word_splits", "run_costs"):
        with pytest.raises(ValueError):
            getattr(plain_crops, name)
    _same(plain_crops, res)
    for k in TABLES:
        assert getattr(plain_crops, k).tobytes() == getattr(res, k).tobytes(), k
    again = f.text_detect_list(crops, GROUPED, want_run_split=True, **WANTS)
    for k in SPLIT_TABLES:
        assert getattr(again, k).tobytes() == getattr(res, k).tobytes(), k
    # a frame call: box glyphs
    uni = f.text_detect(uniform, GROUPED, want_run_split=True, **WANTS)
    check_split(S, f, oracle, uni, [(640, 480)] * 2, labels)
    for k in TABLES:
        assert getattr(plain, k).tobytes() == getattr(uni, k).tobytes(), k
    assert f.run_split_stats()[0] > 0 and f.run_split_stats()[1] > 0
    # SPLIT 0 and 255 on the same frames: other segmentations, the same cuts
    try:
        f.set_run_split(NUM, DEN, 255)
        stiff = f.text_detect_list(crops, GROUPED, want_run_split=True, **WANTS)
        assert stiff.run_pieces.tobytes() == res.run_pieces.tobytes() and (stiff.word_splits["n_parts"] == stiff.words["n_runs"]).all()
        assert (stiff.split_parts["piece"] == -1).all()
    finally:
        f.set_run_split(NUM, DEN, SPLIT)


def test_a_detected_word_splits(scene, oracle, cascade_paths):
    """The issue's second condition: at least one word of the detect calls has n_parts > n_runs.  With the shipped models no word
    splits (the module's docstring has the figures), so the context of this test reads with run_split_ref.prototype_model of the
    frame call's own pieces.  Every table of the flag, the matcher and the decoder are then held on split sequences that are not the
    runs."""
    S, f, prm, path, labels, uniform, crops, plain, plain_crops = scene
    shipped = f.text_detect(uniform, GROUPED, want_run_split=True, **WANTS)
    assert int((shipped.word_splits["n_parts"] > shipped.words["n_runs"]).sum()) == 0
    feet = [(g.x, g.y, g.bits) for g in frame_lines_reference(shipped, [(640, 480)] * 2)[0]]
    tabs, splits, pieces, line_of = RS.tables(feet, NUM, DEN)
    pq, _ = RS.piece_features(oracle, feet, pieces, line_of, [float(t["slope"]) for t in shipped.texts])
    order = sorted(range(len(pieces)), key=lambda k: (pieces[k][2] - pieces[k][1] != 1, k))          # the atoms first: a run splits into known parts
    assert len(order) >= 65
    own = np.arange(65, dtype=np.int64)
    g = S.ERFilter(params=prm)
    try:
        g.load_cascade(0, cascade_paths[0]); g.load_cascade(1, cascade_paths[1])
        g.load_svm_model_text(RS.prototype_model(pq[order[:65]]), 1800)
        g.set_run_split(NUM, DEN, SPLIT)
        res = g.text_detect(uniform, GROUPED, want_run_split=True, **WANTS)
        cut, longer = check_split(S, g, oracle, res, [(640, 480)] * 2, own)
        assert cut >= 5 and longer >= 1
        assert (res.split_parts["piece"] >= 0).any() and (res.word_splits["cost"] < res.word_splits["read_cost"]).any()
        for k in TABLES:
            if k not in ("run_reads",):
                assert getattr(plain, k).tobytes() == getattr(res, k).tobytes(), k
        lst = g.text_detect_list(crops, GROUPED, want_run_split=True, **WANTS)
        check_split(S, g, oracle, lst, [(c.shape[1], c.shape[0]) for c in crops], own)
        both = check_match_decode(S, g, oracle, lambda **kw: g.text_detect(uniform, GROUPED, **kw, **WANTS), [(640, 480)] * 2, own,
                                  [plain.word_text(w) for w in range(len(plain.words))])
        assert (both.word_splits["n_parts"] > both.words["n_runs"]).any()
        # the decoder's sources index the word's parts: a word that split has a source beyond its runs
        d, ws = both.word_decodes, both.word_splits
        for w in np.flatnonzero((d["cost"] >= 0) & (ws["n_parts"] > both.words["n_runs"])):
            src = both.word_decode_src[w, :int(d[w]["n_chars"])] & 0x7F
            assert int(src.max(initial=0)) < int(ws[w]["n_parts"])
    finally:
        g.close()


def check_match_decode(S, f, oracle, detect, sizes, labels, texts):
    """The matcher and the decoder beside the flag on the call detect(**wants): both on the split sequence, every table against
    match_words / decode_words on the parts' rows, with a lexicon that folds and one that does not; returns the result with both."""
    alone = detect(want_run_split=True)
    read = sorted({alone.word_split_text(w) for w in range(len(alone.words))} | set(texts))
    read = [t for t in read if 1 <= len(t) <= 32 and all(ch in WM.ALPHABET for ch in t)]
    table = S.bigram_from_words(read)
    f.set_bigram(table)
    f.set_word_decode(40, 90)
    both = None
    try:
        for fold in (False, True):
            f.set_lexicon(read + ["HOTEL", "hotel"], fold_case=fold)
            both = detect(want_run_split=True, want_word_match=True, want_word_decode=True)
            check_split(S, f, oracle, both, sizes, labels, fold)
            for k in ("run_splits", "run_pieces", "piece_reads", "split_parts", "word_splits"):
                assert getattr(both, k).tobytes() == getattr(alone, k).tobytes(), k
            assert (both.run_costs == WM.cost_rows(both.run_probs, labels, fold)).all()
            ws = both.word_splits
            # the matcher on the parts' rows (folded as the lexicon says)
            m = f.match_words(_part_rows(both), ws["first_part"], ws["n_parts"])
            assert m.tobytes() == both.word_matches.tobytes()
            assert (both.word_matches["free_cost"] == ws["cost"] - SPLIT * (ws["n_parts"] - both.words["n_runs"])).all()
            # the decoder on the parts' unfolded rows: those of the call with the flag alone
            dec, chars, src = f.decode_words(_part_rows(alone), ws["first_part"], ws["n_parts"])
            assert dec.tobytes() == both.word_decodes.tobytes() and chars.tobytes() == both.word_decode_chars.tobytes() and src.tobytes() == both.word_decode_src.tobytes()
            only = detect(want_run_split=True, want_word_decode=True)
            for k in ("word_decodes", "word_decode_chars", "word_decode_src"):
                assert getattr(only, k).tobytes() == getattr(both, k).tobytes(), k
            assert only.piece_costs.tobytes() == alone.piece_costs.tobytes() and only.run_costs.tobytes() == alone.run_costs.tobytes()
            # without the split flag nothing of theirs changes
            unsplit = detect(want_word_match=True, want_word_decode=True)
            m0 = f.match_words(unsplit.run_costs, unsplit.words["first_run"], unsplit.words["n_runs"])
            assert m0.tobytes() == unsplit.word_matches.tobytes() and unsplit.run_costs.tobytes() == both.run_costs.tobytes()
            assert (both.word_decodes["n_sub"] + both.word_decodes["n_del"] == ws["n_parts"])[both.word_decodes["cost"] >= 0].all()
    finally:
        f.set_lexicon([])
        f.set_word_decode()
        f.set_bigram(None)
    return both


def test_matcher_and_decoder_on_the_split_sequence(scene, oracle):
    S, f, prm, path, labels, uniform, crops, plain, plain_crops = scene
    sizes = [(c.shape[1], c.shape[0]) for c in crops]
    check_match_decode(S, f, oracle, lambda **kw: f.text_detect_list(crops, GROUPED, **kw, **WANTS), sizes, labels,
                       [plain_crops.word_text(w) for w in range(len(plain_crops.words))])


def test_stream_and_flag_rules(scene, cascade_paths):
    S, f, prm, path, labels, uniform, crops, plain, plain_crops = scene
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS
    res = f.text_detect_list(crops, GROUPED, want_run_split=True, **WANTS)
    uni = f.text_detect(uniform, GROUPED, want_run_split=True, **WANTS)
    st = S.FrameStream(prm, depth=2)
    try:
        st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
        st.load_svm_model(path, 1800)
        st.set_run_split(NUM, DEN, SPLIT)                                # (on every context of the stream)
        st.submit_copy_list(crops, flags | S.WANT_MASKS, want_run_read=True, want_run_split=True)
        st.submit_copy(uniform, flags | S.WANT_MASKS, want_run_read=True, want_run_split=True)
        _, a = st.next()
        for k in TABLES + SPLIT_TABLES:
            assert getattr(a, k).tobytes() == getattr(res, k).tobytes(), k
        st.submit_copy_list(crops, flags, want_run_read=True)
        _, b = st.next()
        for k in TABLES + SPLIT_TABLES:
            assert getattr(b, k).tobytes() == getattr(uni, k).tobytes(), k
        _, c = st.next()
        with pytest.raises(ValueError):
            c.run_splits
        assert c.run_reads.tobytes() == res.run_reads.tobytes()
    finally:
        st.close()
    # the refusals name the flag and leave the context usable
    with pytest.raises(S.StrErError) as e:                               # without STR_ER_WANT_RUN_READ
        f.text_detect(uniform, flags | S.WANT_RUN_SPLIT)
    assert e.value.code == -1 and "STR_ER_WANT_RUN_SPLIT" in str(e.value)
    planes = f.compute_channels(uniform[0])
    with pytest.raises(S.StrErError) as e:                               # the per-plane calls
        f.detect_planes(planes[:1], S.STAGE_ALL | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS | S.WANT_RUN_READ | S.WANT_RUN_SPLIT)
    assert e.value.code == -1 and "STR_ER_WANT_RUN_SPLIT" in str(e.value)
    for bad in ((0, 4, 8), (1, 0, 8), (65536, 4, 8), (1, 65536, 8), (1, 4, -1), (1, 4, 256)):
        with pytest.raises(S.StrErError) as e:
            f.set_run_split(*bad)
        assert e.value.code == -1
    good = f.text_detect(uniform, GROUPED, want_run_split=True, **WANTS)  # (the parameters are what they were)
    for k in SPLIT_TABLES:
        assert getattr(good, k).tobytes() == getattr(uni, k).tobytes(), k
    # a grouped call without lines: empty tables, not an error
    blank = f.text_detect(np.full((120, 160, 3), 128, np.uint8), flags | S.WANT_RUN_READ | S.WANT_RUN_SPLIT)
    assert len(blank.texts) == 0 and len(blank.run_splits) == len(blank.run_pieces) == len(blank.split_parts) == len(blank.word_splits) == 0
    assert blank.piece_costs.shape == (0, 65) and blank.run_costs.shape == (0, 65)
