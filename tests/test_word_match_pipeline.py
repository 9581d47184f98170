"""STR_ER_WANT_WORD_MATCH in the detect calls, on the frames and the model of test_run_read.py's detect test: the three links of the
stage with == -- run_costs is prob_costs of run_probs, word_matches is the reference (word_match_ref.py) on run_costs and the words,
run_probs at a run's label is its run_reads prob -- the other tables of the result byte for byte those of the call without the flag,
and the same through a list call and a stream submission.  The frames hold box glyphs, not rendered words: the lexicon is what the runs
of the words read (the call without the flag), a few of those strings with a character changed or dropped, and random distractors."""
import numpy as np
import pytest

import word_match_ref as WM
from test_frame_lines import GROUPED, _same
from test_svm_exact import _shipped

pytestmark = pytest.mark.gpu
TABLES = ("line_words", "line_runs", "words", "run_reads", "run_features", "line_feet", "line_pairs", "frame_lines", "frame_line_members", "masks", "mask_bits")
WANTS = dict(want_masks=True, want_frame_lines=True, want_line_words=True, want_run_read=True)


@pytest.fixture(scope="module")
def scene(S, cascade_paths, tmp_path_factory):
    path, m = _shipped(S, tmp_path_factory, 5)
    prm = S.Params(max_width=640, max_height=480, max_frames=2, n_pyr_levels=2)
    f = S.ERFilter(params=prm)
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    f.load_svm_model(path, 1800)
    sy = S.synth
    uniform = np.stack([sy.stext_bgr(sy.frame_seed(2), 640, 480), sy.stext_bgr(sy.frame_seed(976), 640, 480)])
    ragged = [uniform[0], sy.stext_bgr(sy.frame_seed(971), 333, 211)]
    plain = f.text_detect(uniform, GROUPED, **WANTS)
    rng = np.random.default_rng(9)
    read = sorted({plain.word_text(w) for w in range(len(plain.words))})
    read = [t for t in read if 1 <= len(t) <= 32]
    near = [t[:-1] for t in read if len(t) > 2][:40] + [t[:1] + "Z" + t[2:] for t in read if len(t) > 2][:40] + [t.swapcase() for t in read][:40]
    lexicon = read + near + ["".join(rng.choice(list(WM.ALPHABET), int(rng.integers(1, 13)))) for _ in range(300)]
    f.set_lexicon(lexicon)
    yield S, f, prm, path, np.asarray(m.label, np.int64), uniform, ragged, plain, lexicon
    f.close()


def check_links(S, res, labels, lexicon, fold=True, ins=64, dele=64, band=2):
    """The three links of a result with the flag; returns how many words took an entry other than their own reading."""
    n = len(res.line_runs)
    assert res.run_costs.shape == (n, 65) and res.run_probs.shape == (n, len(labels)) and len(res.word_matches) == len(res.words)
    assert (res.run_costs == S.prob_costs(res.run_probs, labels, fold)).all()
    assert (res.run_costs == WM.cost_rows(res.run_probs, labels, fold)).all()
    want = WM.match_words(res.run_costs, res.words["first_run"], res.words["n_runs"], WM.Lexicon(lexicon, fold), ins, dele, band)
    assert WM.as_tuples(res.word_matches) == want
    assert np.array_equal(res.run_probs[np.arange(n), res.run_reads["label"]], res.run_reads["prob"])
    changed = 0
    for w in range(len(res.words)):
        e = int(res.word_matches[w]["entry"])
        assert res.word_match_text(w) == (lexicon[e] if e >= 0 else res.word_text(w))
        changed += res.word_match_text(w) != res.word_text(w)
    for t in range(len(res.line_words)):
        lw = res.line_words[t]
        assert res.words_match_text_of_line(t) == [res.word_match_text(w) for w in range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))]
    for i, g in enumerate(res.frame_lines):
        assert res.frame_line_match_text(i) == " ".join(res.words_match_text_of_line(int(g["rep"])))
    return changed


def test_detect_matches_every_word(scene):
    S, f, prm, path, labels, uniform, ragged, plain, lexicon = scene
    res = f.text_detect(uniform, GROUPED, want_word_match=True, **WANTS)
    assert len(res.words) > 10 and len(res.line_runs) > len(res.words)
    check_links(S, res, labels, lexicon)
    # a word's own reading is in the lexicon, and it costs the word's free cost: the best entry costs no more
    m = res.word_matches
    short = res.words["n_runs"] <= 32
    assert short.any() and (m["cost"][short] <= m["free_cost"][short]).all() and (m["entry"][short] >= 0).all() and (m["n_tried"][short] > 0).all()
    # every other table is that of the call without the flag
    with pytest.raises(ValueError):
        plain.word_matches
    _same(plain, res)
    for k in TABLES:
        assert getattr(plain, k).tobytes() == getattr(res, k).tobytes(), k
    again = f.text_detect(uniform, GROUPED, want_word_match=True, **WANTS)
    for k in ("word_matches", "run_costs", "run_probs"):
        assert getattr(again, k).tobytes() == getattr(res, k).tobytes(), k
    # the matcher's own entry point on the result's cost rows
    assert f.match_words(res.run_costs, res.words["first_run"], res.words["n_runs"]).tobytes() == m.tobytes()
    assert (f.run_costs(res.run_probs) == res.run_costs).all()
    # other parameters, a lexicon without the readings and without fold-case
    f.set_word_match(40, 90, 1)
    f.set_lexicon(lexicon[len(lexicon) - 340:], fold_case=False)
    try:
        other = f.text_detect(uniform, GROUPED, want_word_match=True, **WANTS)
        assert check_links(S, other, labels, lexicon[len(lexicon) - 340:], False, 40, 90, 1) > 0
        assert other.run_reads.tobytes() == res.run_reads.tobytes()
    finally:
        f.set_word_match()
        f.set_lexicon(lexicon)


def test_list_call_and_stream(scene, cascade_paths):
    S, f, prm, path, labels, uniform, ragged, plain, lexicon = scene
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS
    res = f.text_detect(uniform, GROUPED, want_word_match=True, **WANTS)
    lst = f.text_detect_list(ragged, GROUPED, want_word_match=True, **WANTS)
    check_links(S, lst, labels, lexicon)
    assert {int(t["frame"]) for t in lst.texts} == {0, 1}
    lst_plain = f.text_detect_list(ragged, GROUPED, **WANTS)
    for k in TABLES:
        assert getattr(lst_plain, k).tobytes() == getattr(lst, k).tobytes(), k
    st = S.FrameStream(prm, depth=2)
    try:
        st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
        st.load_svm_model(path, 1800)
        st.set_lexicon(lexicon)                                          # (on every context of the stream)
        st.set_word_match(64, 64, 2)
        st.submit_copy(uniform, flags | S.WANT_MASKS, want_run_read=True, want_word_match=True)
        st.submit_copy_list(ragged, flags | S.WANT_MASKS, want_run_read=True, want_word_match=True)
        _, a = st.next()
        for k in TABLES + ("word_matches", "run_costs", "run_probs"):
            assert getattr(a, k).tobytes() == getattr(res, k).tobytes(), k
        assert [a.word_match_text(w) for w in range(len(a.words))] == [res.word_match_text(w) for w in range(len(res.words))]
        st.submit_copy(uniform, flags, want_run_read=True)
        _, b = st.next()
        for k in TABLES + ("word_matches", "run_costs", "run_probs"):
            assert getattr(b, k).tobytes() == getattr(lst, k).tobytes(), k
        _, c = st.next()
        with pytest.raises(ValueError):
            c.word_matches
        assert c.run_reads.tobytes() == res.run_reads.tobytes()
    finally:
        st.close()


def test_flag_rules_leave_the_context_usable(scene):
    S, f, prm, path, labels, uniform, ragged, plain, lexicon = scene
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS
    with pytest.raises(S.StrErError) as e:                               # without STR_ER_WANT_RUN_READ
        f.text_detect(uniform, flags | S.WANT_WORD_MATCH)
    assert e.value.code == -1 and "STR_ER_WANT_WORD_MATCH" in str(e.value)
    planes = f.compute_channels(uniform[0])
    with pytest.raises(S.StrErError) as e:                               # the per-plane calls
        f.detect_planes(planes[:1], S.STAGE_ALL | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS | S.WANT_RUN_READ | S.WANT_WORD_MATCH)
    assert e.value.code == -1 and "STR_ER_WANT_WORD_MATCH" in str(e.value)
    f.set_lexicon([])
    try:
        with pytest.raises(S.StrErError) as e:                           # without a lexicon
            f.text_detect(uniform, flags | S.WANT_RUN_READ | S.WANT_WORD_MATCH)
        assert e.value.code == -6 and "STR_ER_WANT_WORD_MATCH" in str(e.value) and "lexicon" in str(e.value)
        ok = f.text_detect(uniform, GROUPED, **WANTS)                    # the call without the flag needs none
        assert ok.run_reads.tobytes() == plain.run_reads.tobytes()
    finally:
        f.set_lexicon(lexicon)
    # a grouped call without lines: empty tables, not an error
    blank = f.text_detect(np.full((120, 160, 3), 128, np.uint8), flags | S.WANT_RUN_READ | S.WANT_WORD_MATCH)
    assert len(blank.texts) == 0 and len(blank.word_matches) == 0 and blank.run_costs.shape == (0, 65) and blank.run_probs.shape[0] == 0
    good = f.text_detect(uniform, GROUPED, want_word_match=True, **WANTS)
    assert len(good.word_matches) == len(plain.words)
