"""str_er_set_lattice_margin in the detect calls, on the frames and the pieces-made model of test_lattice_decode_pipeline.py (its
fixture): with the setting on the result's margin tables are the stand-alone call (str_er_lattice_margins) on the result's own
run_splits, run_costs and piece_costs, and the numpy reference, with ==, and some word there has a cut margin; with the setting off the
getters are empty, and str_er_lattice_decode_stats and the lattice decoder's bytes are those of a context that never heard of the
setting; the same through a stream."""
import numpy as np
import pytest

import lattice_margin_ref as LM
from test_frame_lines import GROUPED
from test_lattice_decode_pipeline import DEL, INS, LATTICE_TABLES, SPLITS, proto  # noqa: F401  (the fixture)
from test_run_split_pipeline import NUM, DEN, SPLIT, SPLIT_TABLES, scene  # noqa: F401  (the fixture's fixture)
from test_word_match_pipeline import TABLES

pytestmark = pytest.mark.gpu
MARGIN_TABLES = ("lattice_margins", "lattice_read_margins", "lattice_cut_margins", "lattice_part_reads", "lattice_part_alts", "lattice_cut_alts")


@pytest.fixture(scope="module")
def never(proto, cascade_paths):  # noqa: F811
    """A context like the fixture's that never hears of the setting."""
    S, g, prm, model, uniform, crops, base, base_crops, table, read = proto
    n = S.ERFilter(params=prm)
    n.load_cascade(0, cascade_paths[0]); n.load_cascade(1, cascade_paths[1])
    n.load_svm_model(model, 1800)
    n.set_run_split(NUM, DEN, SPLIT)
    n.set_bigram(table)
    n.set_word_decode(INS, DEL)
    yield n
    n.close()


def check_margins(S, g, res, table):
    """The margin tables of a result against the stand-alone call and the reference on the result's own tables, and the accessors;
    returns the number of words with a cut margin."""
    n = len(res.words)
    first, n_of = res.words["first_run"], res.words["n_runs"]
    got = tuple(getattr(res, k) for k in MARGIN_TABLES)
    assert got[0].dtype == S.LATTICE_MARGIN_DTYPE and len(got[0]) == n and all(t.shape == (n, 32) for t in got[1:])
    assert got[1].dtype == got[2].dtype == np.int32 and got[3].dtype == got[4].dtype == got[5].dtype == np.uint8
    alone = g.lattice_margins(res.run_splits, res.run_costs, res.piece_costs, first, n_of)
    want = LM.lattice_margins(res.run_splits, res.run_costs, res.piece_costs, first, n_of, table, INS, DEL, SPLIT)
    assert LM.as_tuples(got[0]) == want[0]
    for k, a, b, c in zip(MARGIN_TABLES, got, alone, (None,) + want[1:6]):
        assert a.tobytes() == b.tobytes(), k
        assert c is None or (a == c).all(), k
    d = res.lattice_decodes
    for w in range(n):
        rec, per_part = res.lattice_margins[w], res.word_lattice_part_margins(w)
        assert res.word_lattice_margin(w) == (int(rec["read_margin"]), int(rec["cut_margin"]))
        if int(d[w]["cost"]) < 0 or int(n_of[w]) == 0:
            assert res.word_lattice_margin(w) == (-1, -1) and per_part == [] and int(rec["n_edges"]) == 0
            continue
        assert len(per_part) == int(d[w]["n_parts"]) == len(res.word_lattice_parts(w))
        assert min(a for a, _ in per_part) == int(rec["read_margin"]) >= 0
        cuts = [b for _, b in per_part if b >= 0]
        assert (min(cuts) if cuts else -1) == int(rec["cut_margin"])
        assert bool(cuts) == bool((res.run_splits["n_cuts"][first[w]:first[w] + n_of[w]] > 0).any())
    with_cut = int((got[0]["cut_margin"] >= 0).sum())
    print(f"{n} words, {int((got[0]['read_margin'] >= 0).sum())} with margins, {with_cut} with a cut margin, "
          f"{int((got[0]['cut_margin'] == 0).sum())} of them 0, {int((got[0]['read_margin'] == 0).sum())} reading margins 0")
    return with_cut


def test_setting_on_the_margins_are_the_stand_alone_call_and_the_reference(proto, never):
    S, g, prm, model, uniform, crops, base, base_crops, table, read = proto
    g.set_lattice_margin(True)
    try:
        res = g.text_detect(uniform, GROUPED, want_lattice_decode=True, **SPLITS)
        assert check_margins(S, g, res, table) >= 1                      # the condition: a word with a cut margin
        # everything else is the call of a context that never had the setting
        ref = never.text_detect(uniform, GROUPED, want_lattice_decode=True, **SPLITS)
        for k in TABLES + SPLIT_TABLES + LATTICE_TABLES:
            assert getattr(ref, k).tobytes() == getattr(res, k).tobytes(), k
        assert g.lattice_decode_stats() == never.lattice_decode_stats() > 0
        again = g.text_detect(uniform, GROUPED, want_lattice_decode=True, **SPLITS)
        for k in MARGIN_TABLES:
            assert getattr(again, k).tobytes() == getattr(res, k).tobytes(), k
        # without the decoder's flag the setting does nothing
        bare = g.text_detect(uniform, GROUPED, **SPLITS)
        for k in MARGIN_TABLES + ("lattice_decodes",):
            with pytest.raises(ValueError):
                getattr(bare, k)
        # beside the word decoder and its margins, and through the list call
        g.set_word_margin(True)
        both = g.text_detect(uniform, GROUPED, want_lattice_decode=True, want_word_decode=True, **SPLITS)
        for k in MARGIN_TABLES + LATTICE_TABLES:
            assert getattr(both, k).tobytes() == getattr(res, k).tobytes(), k
        assert len(both.word_margins) == len(both.words)
        g.set_word_margin(False)
        lst = g.text_detect_list(crops, GROUPED, want_lattice_decode=True, **SPLITS)
        check_margins(S, g, lst, table)
        ref = never.text_detect_list(crops, GROUPED, want_lattice_decode=True, **SPLITS)
        for k in TABLES + SPLIT_TABLES + LATTICE_TABLES:
            assert getattr(ref, k).tobytes() == getattr(lst, k).tobytes(), k
        assert g.lattice_decode_stats() == never.lattice_decode_stats()
        # a grouped call without lines: empty tables, not an error
        blank = g.text_detect(np.full((120, 160, 3), 128, np.uint8), GROUPED, want_lattice_decode=True, **SPLITS)
        assert len(blank.lattice_margins) == 0 and blank.lattice_read_margins.shape == blank.lattice_cut_alts.shape == (0, 32)
    finally:
        g.set_lattice_margin(False)
        g.set_word_margin(False)


def test_setting_off_nothing_is_made_and_nothing_changes(proto, never):
    S, g, prm, model, uniform, crops, base, base_crops, table, read = proto
    g.set_lattice_margin(True)
    g.text_detect(uniform, GROUPED, want_lattice_decode=True, **SPLITS)
    g.set_lattice_margin(False)
    for wants in (dict(want_lattice_decode=True), dict(want_lattice_decode=True, want_word_decode=True)):
        off = g.text_detect(uniform, GROUPED, **wants, **SPLITS)
        ref = never.text_detect(uniform, GROUPED, **wants, **SPLITS)
        for k in MARGIN_TABLES:
            with pytest.raises(ValueError):
                getattr(off, k)
            with pytest.raises(ValueError):
                getattr(ref, k)
        with pytest.raises(ValueError):
            off.word_lattice_margin(0)
        with pytest.raises(ValueError):
            off.word_lattice_part_margins(0)
        for k in TABLES + SPLIT_TABLES + LATTICE_TABLES:
            assert getattr(ref, k).tobytes() == getattr(off, k).tobytes(), k
        assert g.lattice_decode_stats() == never.lattice_decode_stats() > 0


def test_through_a_stream(proto, cascade_paths):
    S, g, prm, model, uniform, crops, base, base_crops, table, read = proto
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS | S.WANT_MASKS
    g.set_lattice_margin(True)
    try:
        res = g.text_detect(uniform, GROUPED, want_lattice_decode=True, **SPLITS)
    finally:
        g.set_lattice_margin(False)
    st = S.FrameStream(prm, depth=2)
    try:
        st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
        st.load_svm_model(model, 1800)
        st.set_run_split(NUM, DEN, SPLIT)
        st.set_bigram(table)
        st.set_word_decode(INS, DEL)
        st.set_lattice_margin(True)                                      # (on every context of the stream)
        st.submit_copy(uniform, flags, want_run_read=True, want_run_split=True, want_lattice_decode=True)
        st.submit_copy(uniform, flags, want_run_read=True, want_run_split=True, want_lattice_decode=True)
        for _ in range(2):
            _, a = st.next()
            for k in TABLES + SPLIT_TABLES + LATTICE_TABLES + MARGIN_TABLES:
                assert getattr(a, k).tobytes() == getattr(res, k).tobytes(), k
        st.set_lattice_margin(False)
        st.submit_copy(uniform, flags, want_run_read=True, want_run_split=True, want_lattice_decode=True)
        _, b = st.next()
        with pytest.raises(ValueError):
            b.lattice_margins
        for k in LATTICE_TABLES:
            assert getattr(b, k).tobytes() == getattr(res, k).tobytes(), k
    finally:
        st.close()
