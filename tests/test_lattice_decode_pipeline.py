"""STR_ER_WANT_LATTICE_DECODE in the detect calls, on the scene of test_run_split_pipeline.py (its fixture; the S-text frames of seeds 2
and 976 and the list of crops) read with a model made from the frame call's own pieces, with which 17 of 22 words split: the flag's
tables are exactly what str_er_lattice_decode_words_host gives on the call's own run_splits, run_costs and piece_costs (no lexicon:
the returned rows are unfolded); the three properties of the contract against the call's own word_decodes and word_splits; every other
table byte for byte that of the call without the flag; the same bytes beside a matcher whose lexicon folds, beside the decoder, through
the list call and through a stream; the flag's rules."""
import numpy as np
import pytest

import run_split_ref as RS
import word_match_ref as WM
from test_frame_lines import GROUPED, reference as frame_lines_reference
from test_run_split_pipeline import NUM, DEN, SPLIT, SPLIT_TABLES, scene  # noqa: F401  (the fixture)
from test_word_match_pipeline import TABLES, WANTS

pytestmark = pytest.mark.gpu
INS, DEL = 40, 90
LATTICE_TABLES = ("lattice_decodes", "lattice_decode_chars", "lattice_decode_src", "lattice_parts")
SPLITS = dict(want_run_split=True, **WANTS)


@pytest.fixture(scope="module")
def proto(scene, oracle, cascade_paths, tmp_path_factory):  # noqa: F811
    """A context that reads with run_split_ref.prototype_model of the frame call's own pieces (atoms first), a bigram table of the words
    it reads, INS / DEL on; the model also as a file, for a stream."""
    S, f, prm, path, labels, uniform, crops, plain, plain_crops = scene
    shipped = f.text_detect(uniform, GROUPED, **SPLITS)
    feet = [(g.x, g.y, g.bits) for g in frame_lines_reference(shipped, [(640, 480)] * 2)[0]]
    tabs, splits, pieces, line_of = RS.tables(feet, NUM, DEN)
    pq, _ = RS.piece_features(oracle, feet, pieces, line_of, [float(t["slope"]) for t in shipped.texts])
    order = sorted(range(len(pieces)), key=lambda k: (pieces[k][2] - pieces[k][1] != 1, k))
    text = RS.prototype_model(pq[order[:65]])
    model = tmp_path_factory.mktemp("lattice") / "prototype.model"
    model.write_bytes(text)
    g = S.ERFilter(params=prm)
    g.load_cascade(0, cascade_paths[0]); g.load_cascade(1, cascade_paths[1])
    g.load_svm_model_text(text, 1800)
    g.set_run_split(NUM, DEN, SPLIT)
    assert g.lattice_decode_stats() == 0
    base = g.text_detect(uniform, GROUPED, **SPLITS)
    base_crops = g.text_detect_list(crops, GROUPED, **SPLITS)
    assert g.lattice_decode_stats() == 0                                 # a call without the flag makes none of the flag's buffers
    read = sorted({base.word_split_text(w) for w in range(len(base.words))} | {base.word_text(w) for w in range(len(base.words))})
    read = [t for t in read if 1 <= len(t) <= 32 and all(ch in WM.ALPHABET for ch in t)]
    table = S.bigram_from_words(read, alpha=0.05)                        # (pairs that were read are cheap: a cut pays where its two characters are a pair)
    g.set_bigram(table)
    g.set_word_decode(INS, DEL)
    yield S, g, prm, str(model), uniform, crops, base, base_crops, table, read
    g.close()


def check_lattice(S, g, res, table):
    """The flag's tables against the host entry point on the call's own rows, the GPU twin, the record identities and the texts; returns
    the number of decoded words with a cut run."""
    first, n_of = res.words["first_run"], res.words["n_runs"]
    hd, hc, hs, hp = S.lattice_decode_words_host(res.run_splits, res.run_costs, res.piece_costs, first, n_of, table, INS, DEL, SPLIT)
    d = res.lattice_decodes
    assert d.dtype == S.LATTICE_DECODE_DTYPE and len(d) == len(res.words) and res.lattice_decode_chars.shape == res.lattice_decode_src.shape == (len(d), 64)
    assert d.tobytes() == hd.tobytes() and res.lattice_decode_chars.tobytes() == hc.tobytes() and res.lattice_decode_src.tobytes() == hs.tobytes()
    assert res.lattice_parts.tobytes() == hp.tobytes()
    gd, gc, gs, gp = g.lattice_decode_words(res.run_splits, res.run_costs, res.piece_costs, first, n_of)
    assert gd.tobytes() == hd.tobytes() and gc.tobytes() == hc.tobytes() and gs.tobytes() == hs.tobytes() and gp.tobytes() == hp.tobytes()
    ok = d["cost"] >= 0
    atoms = np.array([int((res.run_splits["n_cuts"][a:a + k] + 1).sum()) for a, k in zip(first, n_of)], np.int64)
    assert (ok == (atoms <= 32)).all()
    assert (d["cost"] <= d["read_cost"])[ok].all() and (d["n_sub"] + d["n_ins"] == d["n_chars"]).all() and (d["n_sub"] + d["n_del"] == d["n_parts"]).all()
    assert ((n_of <= d["n_parts"]) & (d["n_parts"] <= atoms))[ok].all() and d["first_part"].tolist() == np.concatenate([[0], np.cumsum(d["n_parts"])])[:-1].tolist()
    for w in range(len(d)):
        parts = res.word_lattice_parts(w)
        assert len(parts) == int(d[w]["n_parts"])
        if ok[w]:
            assert res.word_lattice_text(w) == "".join(WM.ALPHABET[int(a)] for a in res.lattice_decode_chars[w, :int(d[w]["n_chars"])])
            assert ((parts["run"] >= first[w]) & (parts["run"] < first[w] + n_of[w])).all()
        else:
            assert res.word_lattice_text(w) == res.word_text(w)
    for i, fl in enumerate(res.frame_lines):
        lw = res.line_words[int(fl["rep"])]
        assert res.frame_line_lattice_text(i) == " ".join(res.word_lattice_text(w) for w in range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"])))
    cut = np.array([bool((res.run_splits["n_cuts"][a:a + k] > 0).any()) for a, k in zip(first, n_of)])
    print(f"{len(d)} words, {int(ok.sum())} decoded, {int((ok & cut).sum())} of them with a cut run, {int((d['n_parts'] > n_of).sum())} with more parts than runs, "
          f"{int((d['cost'] < d['read_cost']).sum())} cheaper than the reading")
    return int((ok & cut).sum())


def test_detect_equals_the_host_on_the_calls_own_rows(proto):
    S, g, prm, model, uniform, crops, base, base_crops, table, read = proto
    res = g.text_detect(uniform, GROUPED, want_lattice_decode=True, **SPLITS)
    assert check_lattice(S, g, res, table) >= 1                          # the condition: a word with a cut run and N <= 32
    assert (res.lattice_parts["piece"] >= 0).any()                       # ... and under this table some word takes pieces of its runs
    assert g.lattice_decode_stats() > 0
    # every other table is that of the call without the flag, which has none of the flag's
    for k in TABLES + SPLIT_TABLES:
        assert getattr(base, k).tobytes() == getattr(res, k).tobytes(), k
    for k in LATTICE_TABLES:
        with pytest.raises(ValueError):
            getattr(base, k)
    again = g.text_detect(uniform, GROUPED, want_lattice_decode=True, **SPLITS)
    for k in LATTICE_TABLES:
        assert getattr(again, k).tobytes() == getattr(res, k).tobytes(), k
    # the list call
    lst = g.text_detect_list(crops, GROUPED, want_lattice_decode=True, **SPLITS)
    check_lattice(S, g, lst, table)
    for k in TABLES + SPLIT_TABLES:
        assert getattr(base_crops, k).tobytes() == getattr(lst, k).tobytes(), k


def test_the_three_properties_against_the_calls_own_decodes_and_splits(proto):
    S, g, prm, model, uniform, crops, base, base_crops, table, read = proto
    alone = g.text_detect(uniform, GROUPED, want_lattice_decode=True, **SPLITS)
    both = g.text_detect(uniform, GROUPED, want_lattice_decode=True, want_word_decode=True, **SPLITS)
    for k in LATTICE_TABLES:                                             # (the decoder's rows instead of the split's own: the same bytes)
        assert getattr(both, k).tobytes() == getattr(alone, k).tobytes(), k
    unsplit = g.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
    d, wd_split, wd_runs, ws = both.lattice_decodes, both.word_decodes, unsplit.word_decodes, both.word_splits
    first, n_of = both.words["first_run"], both.words["n_runs"]
    seen = [0, 0, 0]
    for w in range(len(d)):
        if int(d[w]["cost"]) < 0:
            continue
        cuts = both.run_splits["n_cuts"][first[w]:first[w] + n_of[w]]
        if not (cuts > 0).any():                                         # (1) byte for byte the word decoder on the runs; the parts are the runs
            assert tuple(int(d[w][k]) for k in wd_runs.dtype.names) == tuple(int(v) for v in wd_runs[w])
            assert both.lattice_decode_chars[w].tobytes() == unsplit.word_decode_chars[w].tobytes() and both.lattice_decode_src[w].tobytes() == unsplit.word_decode_src[w].tobytes()
            parts = both.word_lattice_parts(w)
            assert parts["run"].tolist() == list(range(first[w], first[w] + n_of[w])) and (parts["piece"] == -1).all()
            seen[0] += 1
        if int(wd_runs[w]["cost"]) >= 0:                                 # (2)
            assert int(d[w]["cost"]) <= int(wd_runs[w]["cost"]) and int(d[w]["read_cost"]) == int(wd_runs[w]["read_cost"])
            seen[1] += 1
        if int(wd_split[w]["cost"]) >= 0:                                # (3)
            assert int(d[w]["cost"]) <= int(wd_split[w]["cost"]) + SPLIT * (int(ws[w]["n_parts"]) - int(n_of[w]))
            seen[2] += 1
    print("words under property 1, 2, 3:", seen)
    assert seen[1] >= 1 and seen[2] >= 1
    # the other tables of the call are those of the call without this flag
    same = g.text_detect(uniform, GROUPED, want_word_decode=True, **SPLITS)
    for k in TABLES + SPLIT_TABLES + ("word_decodes", "word_decode_chars", "word_decode_src", "run_probs"):
        assert getattr(same, k).tobytes() == getattr(both, k).tobytes(), k


def test_beside_the_matcher_the_bytes_are_the_same(proto):
    S, g, prm, model, uniform, crops, base, base_crops, table, read = proto
    alone = g.text_detect(uniform, GROUPED, want_lattice_decode=True, **SPLITS)
    try:
        for fold in (True, False):
            g.set_lexicon(read + ["HOTEL", "hotel"], fold_case=fold)
            for more in (dict(want_word_match=True), dict(want_word_match=True, want_word_decode=True)):
                res = g.text_detect(uniform, GROUPED, want_lattice_decode=True, **more, **SPLITS)
                for k in LATTICE_TABLES:
                    assert getattr(res, k).tobytes() == getattr(alone, k).tobytes(), (fold, more, k)
                plain = g.text_detect(uniform, GROUPED, **more, **SPLITS)   # ... and the matcher's and the decoder's are what they are without this flag
                for k in TABLES + SPLIT_TABLES + ("word_matches", "run_probs") + (("word_decodes", "word_decode_chars", "word_decode_src") if len(more) > 1 else ()):
                    assert getattr(plain, k).tobytes() == getattr(res, k).tobytes(), (fold, more, k)
            if fold:
                assert (res.piece_costs != alone.piece_costs).any()      # (the returned rows are folded here: the lattice read rows of its own)
    finally:
        g.set_lexicon([])


def test_stream_and_flag_rules(proto, cascade_paths):
    S, g, prm, model, uniform, crops, base, base_crops, table, read = proto
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS
    res = g.text_detect_list(crops, GROUPED, want_lattice_decode=True, **SPLITS)
    uni = g.text_detect(uniform, GROUPED, want_lattice_decode=True, **SPLITS)
    st = S.FrameStream(prm, depth=2)
    try:
        st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
        st.load_svm_model(model, 1800)
        st.set_run_split(NUM, DEN, SPLIT)                                # (on every context of the stream)
        st.set_bigram(table)
        st.set_word_decode(INS, DEL)
        st.submit_copy_list(crops, flags | S.WANT_MASKS, want_run_read=True, want_run_split=True, want_lattice_decode=True)
        st.submit_copy(uniform, flags | S.WANT_MASKS, want_run_read=True, want_run_split=True, want_lattice_decode=True)
        _, a = st.next()
        for k in TABLES + SPLIT_TABLES + LATTICE_TABLES:
            assert getattr(a, k).tobytes() == getattr(res, k).tobytes(), k
        st.submit_copy_list(crops, flags, want_run_read=True, want_run_split=True)
        _, b = st.next()
        for k in TABLES + SPLIT_TABLES + LATTICE_TABLES:
            assert getattr(b, k).tobytes() == getattr(uni, k).tobytes(), k
        _, c = st.next()
        with pytest.raises(ValueError):
            c.lattice_decodes
        assert c.run_splits.tobytes() == res.run_splits.tobytes()
    finally:
        st.close()
    # the refusals name the flag and leave the context usable
    want = flags | S.WANT_RUN_READ | S.WANT_RUN_SPLIT | S.WANT_LATTICE_DECODE
    with pytest.raises(S.StrErError) as e:                               # without STR_ER_WANT_RUN_SPLIT
        g.text_detect(uniform, want & ~S.WANT_RUN_SPLIT)
    assert e.value.code == -1 and "STR_ER_WANT_LATTICE_DECODE" in str(e.value) and "STR_ER_WANT_RUN_SPLIT" in str(e.value)
    with pytest.raises(S.StrErError) as e:                               # ... nor STR_ER_WANT_RUN_READ
        g.text_detect(uniform, want & ~S.WANT_RUN_READ & ~S.WANT_RUN_SPLIT)
    assert e.value.code == -1 and "STR_ER_WANT_LATTICE_DECODE" in str(e.value)
    planes = g.compute_channels(uniform[0])
    with pytest.raises(S.StrErError) as e:                               # the per-plane calls
        g.detect_planes(planes[:1], S.STAGE_ALL | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS | S.WANT_RUN_READ | S.WANT_RUN_SPLIT | S.WANT_LATTICE_DECODE)
    assert e.value.code == -1 and "STR_ER_WANT_LATTICE_DECODE" in str(e.value)
    with pytest.raises(S.StrErError) as e:                               # the strip path (the flags are judged before the blobs are read)
        g.strip_merge(uniform[0], [b"none"], stages=want)
    assert e.value.code == -1 and "STR_ER_WANT_LATTICE_DECODE" in str(e.value) and "strip" in str(e.value)
    g.set_bigram(None)
    try:
        with pytest.raises(S.StrErError) as e:                           # no table
            g.text_detect(uniform, want)
        assert e.value.code == -6 and "STR_ER_WANT_LATTICE_DECODE" in str(e.value) and "bigram" in str(e.value)
    finally:
        g.set_bigram(table)
    good = g.text_detect(uniform, GROUPED, want_lattice_decode=True, **SPLITS)  # (the context is usable afterwards)
    for k in SPLIT_TABLES + LATTICE_TABLES:
        assert getattr(good, k).tobytes() == getattr(uni, k).tobytes(), k
    # a grouped call without lines: empty tables, not an error
    blank = g.text_detect(np.full((120, 160, 3), 128, np.uint8), want)
    assert len(blank.texts) == 0 and len(blank.lattice_decodes) == len(blank.lattice_parts) == 0
    assert blank.lattice_decode_chars.shape == blank.lattice_decode_src.shape == (0, 64)
