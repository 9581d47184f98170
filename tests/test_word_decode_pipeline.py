"""STR_ER_WANT_WORD_DECODE in the detect calls, on the frames, the model and the flags of test_word_match_pipeline.py: run_costs is
the unfolded prob_costs of run_probs, the decode tables are the reference (word_decode_ref.py) and decode_words on the result's rows,
the texts and word_decode_runs agree with the tables, every other table of the result is byte for byte that of the call without the
flag, and the same through a list call and a stream submission.  The frames hold box glyphs, not rendered words: one table is
bigram_from_words of what the runs of the words read (the call without the flag), the other is random."""
import numpy as np
import pytest

import word_decode_ref as WD
import word_match_ref as WM
from test_frame_lines import GROUPED, _same
from test_svm_exact import _shipped
from test_word_match_pipeline import TABLES, WANTS

pytestmark = pytest.mark.gpu
DECODE_TABLES = ("word_decodes", "word_decode_chars", "word_decode_src", "run_costs", "run_probs")
MATCH_TABLES = ("word_matches", "run_costs", "run_probs")


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
    read = sorted({plain.word_text(w) for w in range(len(plain.words))})
    read = [t for t in read if t and all(ch in WM.ALPHABET for ch in t)]
    table = S.bigram_from_words(read)
    random_table = np.random.default_rng(9).integers(0, 256, (66, 66)).astype(np.uint8)
    f.set_bigram(table)
    yield S, f, prm, path, np.asarray(m.label, np.int64), uniform, ragged, plain, table, random_table, read
    f.close()


def check_links(S, f, res, labels, table, ins=0, dele=0):
    """The links of a result with the flag alone; returns how many words read otherwise than their runs' arg max."""
    n = len(res.line_runs)
    assert res.run_costs.shape == (n, 65) and res.run_probs.shape == (n, len(labels)) and len(res.word_decodes) == len(res.words)
    assert res.word_decode_chars.shape == res.word_decode_src.shape == (len(res.words), 64)
    assert (res.run_costs == S.prob_costs(res.run_probs, labels, False)).all()
    assert (res.run_costs == WM.cost_rows(res.run_probs, labels, False)).all()
    want, wc, ws = WD.decode_words(res.run_costs, res.words["first_run"], res.words["n_runs"], table, ins, dele)
    assert WD.as_tuples(res.word_decodes) == want
    assert (res.word_decode_chars == wc).all() and (res.word_decode_src == ws).all()
    dec, chars, src = f.decode_words(res.run_costs, res.words["first_run"], res.words["n_runs"])
    assert dec.tobytes() == res.word_decodes.tobytes() and chars.tobytes() == res.word_decode_chars.tobytes() and src.tobytes() == res.word_decode_src.tobytes()
    assert np.array_equal(res.run_probs[np.arange(n), res.run_reads["label"]], res.run_reads["prob"])
    changed = 0
    for w in range(len(res.words)):
        d, word = res.word_decodes[w], res.words[w]
        text, runs = res.word_decode_text(w), res.word_decode_runs(w)
        if int(d["cost"]) < 0:
            assert text == res.word_text(w) and runs == [(int(word["first_run"]) + k, False) for k in range(int(word["n_runs"]))]
        else:
            assert text == "".join(WM.ALPHABET[a] for a in res.word_decode_chars[w, :int(d["n_chars"])])
            assert len(runs) == len(text) == int(d["n_chars"]) and sum(ins_ for _, ins_ in runs) == int(d["n_ins"])
            first = int(word["first_run"])
            assert all(first <= i < first + int(word["n_runs"]) for i, _ in runs) and [i for i, _ in runs] == sorted(i for i, _ in runs)
            assert int(d["cost"]) <= int(d["read_cost"]) and int(d["n_sub"]) + int(d["n_del"]) == int(word["n_runs"])
        changed += text != res.word_text(w)
    for t in range(len(res.line_words)):
        lw = res.line_words[t]
        assert res.words_decode_text_of_line(t) == [res.word_decode_text(w) for w in range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))]
    for i, g in enumerate(res.frame_lines):
        assert res.frame_line_decode_text(i) == " ".join(res.words_decode_text_of_line(int(g["rep"])))
    return changed


def test_detect_decodes_every_word(scene):
    S, f, prm, path, labels, uniform, ragged, plain, table, random_table, read = scene
    res = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
    assert len(res.words) > 10 and len(res.line_runs) > len(res.words)
    check_links(S, f, res, labels, table)
    # every other table is that of the call without the flag
    for name in ("word_decodes", "word_decode_chars", "word_decode_src", "run_costs", "word_matches"):
        with pytest.raises(ValueError):
            getattr(plain, name)
    with pytest.raises(ValueError):
        res.word_matches
    _same(plain, res)
    for k in TABLES:
        assert getattr(plain, k).tobytes() == getattr(res, k).tobytes(), k
    again = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
    for k in DECODE_TABLES:
        assert getattr(again, k).tobytes() == getattr(res, k).tobytes(), k
    # the moves on, and a random table
    try:
        f.set_word_decode(40, 90)
        check_links(S, f, f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS), labels, table, 40, 90)
        f.set_bigram(random_table)
        f.set_word_decode(8, 8)
        other = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
        assert check_links(S, f, other, labels, random_table, 8, 8) > 0
        assert other.run_reads.tobytes() == res.run_reads.tobytes() and other.run_costs.tobytes() == res.run_costs.tobytes()
    finally:
        f.set_word_decode()
        f.set_bigram(table)


def test_both_flags_with_a_fold_case_lexicon(scene):
    S, f, prm, path, labels, uniform, ragged, plain, table, random_table, read = scene
    lexicon = [t for t in read if 1 <= len(t) <= 32] + ["HOTEL", "hotel"]
    only_decode = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
    f.set_lexicon(lexicon, fold_case=True)
    try:
        only_match = f.text_detect(uniform, GROUPED, want_word_match=True, **WANTS)
        both = f.text_detect(uniform, GROUPED, want_word_match=True, want_word_decode=True, **WANTS)
        for k in MATCH_TABLES:                                           # the matcher's, folded: that call's bytes do not change
            assert getattr(both, k).tobytes() == getattr(only_match, k).tobytes(), k
        assert (both.run_costs == WM.cost_rows(both.run_probs, labels, True)).all()
        assert both.run_costs.tobytes() != only_decode.run_costs.tobytes()           # (the model has both cases: folding changes rows)
        for k in ("word_decodes", "word_decode_chars", "word_decode_src", "run_probs"):
            assert getattr(both, k).tobytes() == getattr(only_decode, k).tobytes(), k
        for k in TABLES:
            assert getattr(both, k).tobytes() == getattr(plain, k).tobytes(), k
        # a lexicon that does not fold: one set of rows serves both
        f.set_lexicon(lexicon, fold_case=False)
        both = f.text_detect(uniform, GROUPED, want_word_match=True, want_word_decode=True, **WANTS)
        assert both.run_costs.tobytes() == only_decode.run_costs.tobytes()
        for k in ("word_decodes", "word_decode_chars", "word_decode_src"):
            assert getattr(both, k).tobytes() == getattr(only_decode, k).tobytes(), k
    finally:
        f.set_lexicon([])


def test_list_call_and_stream(scene, cascade_paths):
    S, f, prm, path, labels, uniform, ragged, plain, table, random_table, read = scene
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS
    res = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
    lst = f.text_detect_list(ragged, GROUPED, want_word_decode=True, **WANTS)
    check_links(S, f, lst, labels, table)
    assert {int(t["frame"]) for t in lst.texts} == {0, 1}
    lst_plain = f.text_detect_list(ragged, GROUPED, **WANTS)
    for k in TABLES:
        assert getattr(lst_plain, k).tobytes() == getattr(lst, k).tobytes(), k
    st = S.FrameStream(prm, depth=2)
    try:
        st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
        st.load_svm_model(path, 1800)
        st.set_bigram(table)                                             # (on every context of the stream)
        st.set_word_decode(0, 0)
        st.submit_copy(uniform, flags | S.WANT_MASKS, want_run_read=True, want_word_decode=True)
        st.submit_copy_list(ragged, flags | S.WANT_MASKS, want_run_read=True, want_word_decode=True)
        _, a = st.next()
        for k in TABLES + DECODE_TABLES:
            assert getattr(a, k).tobytes() == getattr(res, k).tobytes(), k
        assert [a.word_decode_text(w) for w in range(len(a.words))] == [res.word_decode_text(w) for w in range(len(res.words))]
        st.submit_copy(uniform, flags, want_run_read=True)
        _, b = st.next()
        for k in TABLES + DECODE_TABLES:
            assert getattr(b, k).tobytes() == getattr(lst, k).tobytes(), k
        _, c = st.next()
        with pytest.raises(ValueError):
            c.word_decodes
        assert c.run_reads.tobytes() == res.run_reads.tobytes()
    finally:
        st.close()


def test_flag_rules_leave_the_context_usable(scene):
    S, f, prm, path, labels, uniform, ragged, plain, table, random_table, read = scene
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS
    with pytest.raises(S.StrErError) as e:                               # without STR_ER_WANT_RUN_READ
        f.text_detect(uniform, flags | S.WANT_WORD_DECODE)
    assert e.value.code == -1 and "STR_ER_WANT_WORD_DECODE" in str(e.value)
    planes = f.compute_channels(uniform[0])
    with pytest.raises(S.StrErError) as e:                               # the per-plane calls
        f.detect_planes(planes[:1], S.STAGE_ALL | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS | S.WANT_RUN_READ | S.WANT_WORD_DECODE)
    assert e.value.code == -1 and "STR_ER_WANT_WORD_DECODE" in str(e.value)
    f.set_bigram(None)
    try:
        with pytest.raises(S.StrErError) as e:                           # without a table
            f.text_detect(uniform, flags | S.WANT_RUN_READ | S.WANT_WORD_DECODE)
        assert e.value.code == -6 and "STR_ER_WANT_WORD_DECODE" in str(e.value) and "bigram" in str(e.value)
        ok = f.text_detect(uniform, GROUPED, **WANTS)                    # the call without the flag needs none
        assert ok.run_reads.tobytes() == plain.run_reads.tobytes()
    finally:
        f.set_bigram(table)
    # a grouped call without lines: empty tables, not an error
    blank = f.text_detect(np.full((120, 160, 3), 128, np.uint8), flags | S.WANT_RUN_READ | S.WANT_WORD_DECODE)
    assert len(blank.texts) == 0 and len(blank.word_decodes) == 0 and blank.word_decode_chars.shape == (0, 64) and blank.word_decode_src.shape == (0, 64)
    assert blank.run_costs.shape == (0, 65) and blank.run_probs.shape[0] == 0
    good = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
    assert len(good.word_decodes) == len(plain.words)
