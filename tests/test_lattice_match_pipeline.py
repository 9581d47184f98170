"""STR_ER_WANT_LATTICE_MATCH in the detect calls, on the scene of test_run_split_pipeline.py read with the prototype model of
test_lattice_decode_pipeline.py (its fixture: a model made from the frame call's own pieces, with which most words split) and a lexicon of
the strings the call reads: the flag's tables are exactly what str_er_lattice_match_words_host gives on the call's own run_splits,
run_costs, piece_costs and words; the three properties of the contract against the same call's word_matches and word_splits and against
match_words on the unsplit runs; every other table byte for byte that of the call without the flag; the list call and a stream; the
flag's rules."""
import numpy as np
import pytest

import word_match_ref as WM
from test_frame_lines import GROUPED
from test_lattice_decode_pipeline import proto  # noqa: F401  (the fixture)
from test_run_split_pipeline import NUM, DEN, SPLIT, SPLIT_TABLES, scene  # noqa: F401  (the fixture)
from test_word_match_pipeline import TABLES, WANTS

pytestmark = pytest.mark.gpu
INS, DEL, BAND = 40, 90, 2
MATCH_TABLES = ("lattice_matches", "lattice_match_src", "lattice_match_parts")
OTHER_TABLES = TABLES + SPLIT_TABLES + ("word_matches", "run_probs")
BOTH = dict(want_run_split=True, want_word_match=True, **WANTS)


@pytest.fixture(scope="module")
def lex(proto):  # noqa: F811
    """The context of the prototype model with a lexicon of the strings it reads (whole runs and split sequences) and a few that it
    does not, INS / DEL / band set; the lexicon is cleared afterwards."""
    S, g, prm, model, uniform, crops, base, base_crops, table, read = proto
    words = read + ["HOTEL", "hotel", "rn", "m", "Zz9", "a" * 32]
    g.set_lexicon(words, fold_case=True)
    g.set_word_match(INS, DEL, BAND)
    yield S, g, prm, model, uniform, crops, words
    g.set_lexicon([])
    g.set_word_match()


def check_match(S, g, res, words, fold=True):
    """The flag's tables against the host entry point on the call's own rows and the GPU twin, the record identities and the texts;
    returns the number of words with a cut run for which an entry was found."""
    first, n_of = res.words["first_run"], res.words["n_runs"]
    hr, hs, hp = S.lattice_match_words_host(res.run_splits, res.run_costs, res.piece_costs, first, n_of, words, fold, INS, DEL, BAND, SPLIT)
    d = res.lattice_matches
    assert d.dtype == S.LATTICE_MATCH_DTYPE and len(d) == len(res.words) and res.lattice_match_src.shape == (len(d), 32)
    assert d.tobytes() == hr.tobytes() and res.lattice_match_src.tobytes() == hs.tobytes() and res.lattice_match_parts.tobytes() == hp.tobytes()
    gr, gs, gp = g.lattice_match_words(res.run_splits, res.run_costs, res.piece_costs, first, n_of)
    assert gr.tobytes() == hr.tobytes() and gs.tobytes() == hs.tobytes() and gp.tobytes() == hp.tobytes()
    ok = d["entry"] >= 0
    atoms = np.array([int((res.run_splits["n_cuts"][a:a + k] + 1).sum()) for a, k in zip(first, n_of)], np.int64)
    assert (d["n_tried"][atoms > 32] == 0).all() and d["first_part"].tolist() == np.concatenate([[0], np.cumsum(d["n_parts"])])[:-1].tolist()
    assert ((n_of <= d["n_parts"]) & (d["n_parts"] <= atoms))[ok].all() and (d["n_parts"][~ok] == 0).all()
    assert (d["free_cost"] == res.word_splits["cost"]).all()                # free_cost is the word's str_er_word_split cost
    for w in range(len(d)):
        parts = res.word_lattice_match_parts(w)
        assert len(parts) == int(d[w]["n_parts"])
        if ok[w]:
            e = words[int(d[w]["entry"])]
            assert res.word_lattice_match_text(w) == e and int(d[w]["n_parts"]) - int(d[w]["n_del"]) + int(d[w]["n_ins"]) == len(e)
            assert ((parts["run"] >= first[w]) & (parts["run"] < first[w] + n_of[w])).all()
            assert (res.lattice_match_src[w, len(e):] == 255).all() and (res.lattice_match_src[w, :len(e)] != 255).all()
        else:
            assert res.word_lattice_match_text(w) == res.word_text(w) and (res.lattice_match_src[w] == 255).all()
    for i, fl in enumerate(res.frame_lines):
        lw = res.line_words[int(fl["rep"])]
        assert res.frame_line_lattice_match_text(i) == " ".join(res.word_lattice_match_text(w) for w in range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"])))
    cut = np.array([bool((res.run_splits["n_cuts"][a:a + k] > 0).any()) for a, k in zip(first, n_of)])
    print(f"{len(d)} words, {int(ok.sum())} matched, {int((ok & cut).sum())} of them with a cut run, {int((d['n_parts'] > n_of).sum())} with more parts than runs")
    return int((ok & cut).sum())


def test_detect_equals_the_host_on_the_calls_own_rows(lex):
    S, g, prm, model, uniform, crops, words = lex
    base = g.text_detect(uniform, GROUPED, **BOTH)
    stats = g.lattice_match_stats()
    res = g.text_detect(uniform, GROUPED, want_lattice_match=True, **BOTH)
    assert check_match(S, g, res, words) >= 3                            # the condition: words with a cut run that are matched
    assert g.lattice_match_stats() > 0 and stats == 0                    # (a call without the flag makes none of the flag's buffers)
    # every other table is that of the call without the flag, which has none of the flag's
    for k in OTHER_TABLES:
        assert getattr(base, k).tobytes() == getattr(res, k).tobytes(), k
    for k in MATCH_TABLES:
        with pytest.raises(ValueError):
            getattr(base, k)
    again = g.text_detect(uniform, GROUPED, want_lattice_match=True, **BOTH)
    for k in MATCH_TABLES:
        assert getattr(again, k).tobytes() == getattr(res, k).tobytes(), k
    # beside the decoder and the lattice decode (rows of their own where the lexicon folds): the same bytes
    more = g.text_detect(uniform, GROUPED, want_lattice_match=True, want_word_decode=True, want_lattice_decode=True, **BOTH)
    for k in MATCH_TABLES + OTHER_TABLES:
        assert getattr(more, k).tobytes() == getattr(res, k).tobytes(), k
    # the list call
    base_crops = g.text_detect_list(crops, GROUPED, **BOTH)
    lst = g.text_detect_list(crops, GROUPED, want_lattice_match=True, **BOTH)
    check_match(S, g, lst, words)
    for k in OTHER_TABLES:
        assert getattr(base_crops, k).tobytes() == getattr(lst, k).tobytes(), k
    # a lexicon that does not fold
    try:
        g.set_lexicon(words, fold_case=False)
        check_match(S, g, g.text_detect(uniform, GROUPED, want_lattice_match=True, **BOTH), words, fold=False)
    finally:
        g.set_lexicon(words, fold_case=True)


def test_the_three_properties_against_the_calls_own_matches_and_splits(lex):
    S, g, prm, model, uniform, crops, words = lex
    res = g.text_detect(uniform, GROUPED, want_lattice_match=True, **BOTH)
    d, wm_split, ws = res.lattice_matches, res.word_matches, res.word_splits
    first, n_of = res.words["first_run"], res.words["n_runs"]
    wm_runs = g.match_words(res.run_costs, first, n_of)                   # the matcher on the unsplit runs
    seen = [0, 0, 0]
    for w in range(len(d)):
        cuts = res.run_splits["n_cuts"][first[w]:first[w] + n_of[w]]
        if not (cuts > 0).any():                                         # (1) field for field the matcher on the runs; the parts are the runs
            assert tuple(int(d[w][k]) for k in WM.MATCH_FIELDS) == WM.as_tuples(wm_runs[w:w + 1])[0] == WM.as_tuples(wm_split[w:w + 1])[0]
            if int(d[w]["entry"]) >= 0:
                parts = res.word_lattice_match_parts(w)
                assert parts["run"].tolist() == list(range(first[w], first[w] + n_of[w])) and (parts["piece"] == -1).all()
            seen[0] += 1
        if int(wm_runs[w]["entry"]) >= 0:                                # (2)
            assert 0 <= int(d[w]["cost"]) <= int(wm_runs[w]["cost"]) and int(d[w]["n_tried"]) >= int(wm_runs[w]["n_tried"])
            seen[1] += 1
        if int(wm_split[w]["entry"]) >= 0 and int((cuts + 1).sum()) <= 32:      # (3)
            assert 0 <= int(d[w]["cost"]) <= int(wm_split[w]["cost"]) + SPLIT * (int(ws[w]["n_parts"]) - int(n_of[w]))
            assert int(d[w]["n_tried"]) >= int(wm_split[w]["n_tried"])
            seen[2] += 1
    print("words under property 1, 2, 3:", seen, "cheaper than the split sequence:",
          int(sum(1 for w in range(len(d)) if wm_split[w]["entry"] >= 0 and d[w]["cost"] < wm_split[w]["cost"] + SPLIT * (ws[w]["n_parts"] - n_of[w]))))
    assert seen[1] >= 3 and seen[2] >= 3


def test_stream_and_flag_rules(lex, cascade_paths):
    S, g, prm, model, uniform, crops, words = lex
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS
    res = g.text_detect_list(crops, GROUPED, want_lattice_match=True, **BOTH)
    uni = g.text_detect(uniform, GROUPED, want_lattice_match=True, **BOTH)
    st = S.FrameStream(prm, depth=2)
    try:
        st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
        st.load_svm_model(model, 1800)
        st.set_run_split(NUM, DEN, SPLIT)                                # (on every context of the stream)
        st.set_lexicon(words)
        st.set_word_match(INS, DEL, BAND)
        more = dict(want_run_read=True, want_run_split=True, want_word_match=True)
        st.submit_copy_list(crops, flags | S.WANT_MASKS, want_lattice_match=True, **more)
        st.submit_copy(uniform, flags | S.WANT_MASKS, want_lattice_match=True, **more)
        _, a = st.next()
        for k in OTHER_TABLES + MATCH_TABLES:
            assert getattr(a, k).tobytes() == getattr(res, k).tobytes(), k
        st.submit_copy_list(crops, flags, **more)
        _, b = st.next()
        for k in OTHER_TABLES + MATCH_TABLES:
            assert getattr(b, k).tobytes() == getattr(uni, k).tobytes(), k
        _, c = st.next()
        with pytest.raises(ValueError):
            c.lattice_matches
        assert c.word_matches.tobytes() == res.word_matches.tobytes()
    finally:
        st.close()
    # the refusals name the flag and leave the context usable
    want = flags | S.WANT_RUN_READ | S.WANT_RUN_SPLIT | S.WANT_WORD_MATCH | S.WANT_LATTICE_MATCH
    with pytest.raises(S.StrErError) as e:                               # without STR_ER_WANT_RUN_SPLIT
        g.text_detect(uniform, want & ~S.WANT_RUN_SPLIT)
    assert e.value.code == -1 and "STR_ER_WANT_LATTICE_MATCH" in str(e.value) and "STR_ER_WANT_RUN_SPLIT" in str(e.value)
    with pytest.raises(S.StrErError) as e:                               # without STR_ER_WANT_WORD_MATCH
        g.text_detect(uniform, want & ~S.WANT_WORD_MATCH)
    assert e.value.code == -1 and "STR_ER_WANT_LATTICE_MATCH" in str(e.value) and "STR_ER_WANT_WORD_MATCH" in str(e.value)
    planes = g.compute_channels(uniform[0])
    with pytest.raises(S.StrErError) as e:                               # the per-plane calls
        g.detect_planes(planes[:1], S.STAGE_ALL | (want & ~GROUPED))
    assert e.value.code == -1 and "STR_ER_WANT_LATTICE_MATCH" in str(e.value)
    with pytest.raises(S.StrErError) as e:                               # the strip path (the flags are judged before the blobs are read)
        g.strip_merge(uniform[0], [b"none"], stages=want)
    assert e.value.code == -1 and "STR_ER_WANT_LATTICE_MATCH" in str(e.value) and "strip" in str(e.value)
    g.set_lexicon([])
    try:
        with pytest.raises(S.StrErError) as e:                           # no lexicon: the matcher's rule
            g.text_detect(uniform, want)
        assert e.value.code == -6 and "lexicon" in str(e.value)
    finally:
        g.set_lexicon(words)
    good = g.text_detect(uniform, GROUPED, want_lattice_match=True, **BOTH)     # (the context is usable afterwards)
    for k in OTHER_TABLES + MATCH_TABLES:
        assert getattr(good, k).tobytes() == getattr(uni, k).tobytes(), k
    # a grouped call without lines: empty tables, not an error
    blank = g.text_detect(np.full((120, 160, 3), 128, np.uint8), want)
    assert len(blank.texts) == 0 and len(blank.lattice_matches) == len(blank.lattice_match_parts) == 0 and blank.lattice_match_src.shape == (0, 32)
