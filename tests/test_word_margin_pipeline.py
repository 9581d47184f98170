"""str_er_set_word_margin in the detect calls, on the frames, the model and the flags of test_word_decode_pipeline.py: with the setting
on the result's margin tables are str_er_word_margins_host on the result's own cost rows and words with == -- the runs' rows, and with
STR_ER_WANT_RUN_SPLIT the rows of the words' parts -- and the accessors agree with the tables; with the setting off the accessors raise
and every other table is byte for byte that of the same call on a context that never had the setting; once through a stream."""
import numpy as np
import pytest

import word_match_ref as WM
from test_frame_lines import GROUPED, _same
from test_run_split_pipeline import _part_rows
from test_svm_exact import _shipped
from test_word_decode_pipeline import DECODE_TABLES
from test_word_match_pipeline import TABLES, WANTS

pytestmark = pytest.mark.gpu
MARGIN_TABLES = ("word_margins", "word_row_margins", "word_row_reads", "word_row_alts")
SPLIT_TABLES = ("run_splits", "run_pieces", "piece_reads", "piece_costs", "split_parts", "word_splits")


@pytest.fixture(scope="module")
def scene(S, cascade_paths, tmp_path_factory):
    path, m = _shipped(S, tmp_path_factory, 5)
    prm = S.Params(max_width=640, max_height=480, max_frames=2, n_pyr_levels=2)
    pair = []
    for _ in range(2):                                   # [0]: the setting goes on and off; [1]: never had it
        f = S.ERFilter(params=prm)
        f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
        f.load_svm_model(path, 1800)
        pair.append(f)
    sy = S.synth
    uniform = np.stack([sy.stext_bgr(sy.frame_seed(2), 640, 480), sy.stext_bgr(sy.frame_seed(976), 640, 480)])
    plain = pair[1].text_detect(uniform, GROUPED, **WANTS)
    read = sorted({plain.word_text(w) for w in range(len(plain.words))})
    table = S.bigram_from_words([t for t in read if t and all(ch in WM.ALPHABET for ch in t)])
    for f in pair:
        f.set_bigram(table)
    yield S, pair[0], pair[1], prm, path, uniform, table
    for f in pair:
        f.close()


def check_margins(S, res, rows, first, n_of, table, ins, dele):
    """The margin tables of a result against the host entry point on the rows and words the decoder read, and the accessors."""
    n = len(res.words)
    rec, rm, rr, ra, _ = S.word_margins_host(rows, first, n_of, table, ins, dele)
    assert res.word_margins.dtype == S.WORD_MARGIN_DTYPE and len(res.word_margins) == n
    assert res.word_row_margins.shape == res.word_row_reads.shape == res.word_row_alts.shape == (n, 32) and res.word_row_margins.dtype == np.int32
    assert res.word_margins.tobytes() == rec.tobytes()
    assert (res.word_row_margins == rm).all() and (res.word_row_reads == rr).all() and (res.word_row_alts == ra).all()
    decided = 0
    for w in range(n):
        d, g = res.word_decodes[w], res.word_margins[w]
        per_char = res.word_decode_char_margins(w)
        assert res.word_decode_margin(w) == int(g["margin"]) and len(per_char) == len(res.word_decode_runs(w))
        if int(d["cost"]) < 0 or int(n_of[w]) == 0:
            assert int(g["margin"]) == -1 and set(per_char) <= {-1}
            continue
        src = res.word_decode_src[w, :int(d["n_chars"])]
        assert per_char == [-1 if int(v) & 0x80 else int(rm[w, int(v)]) for v in src]
        own = [v for v, s in zip(per_char, src) if not int(s) & 0x80]
        assert all(v >= int(g["margin"]) >= 0 for v in own) and per_char.count(-1) == int(d["n_ins"])
        assert int(g["read"]) == int(rr[w, int(g["row"])]) and int(g["alt"]) == int(ra[w, int(g["row"])]) != int(g["read"])
        decided += int(g["margin"]) > 0
    return decided


def test_setting_on_the_margins_are_the_host_rules_on_the_result_s_rows(scene):
    S, f, never, prm, path, uniform, table = scene
    f.set_word_margin(True)
    try:
        res = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
        assert len(res.words) > 10
        assert check_margins(S, res, res.run_costs, res.words["first_run"], res.words["n_runs"], table, 0, 0) > 0
        # everything else is the call of a context that never had the setting
        ref = never.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
        _same(ref, res)
        for k in TABLES + DECODE_TABLES:
            assert getattr(ref, k).tobytes() == getattr(res, k).tobytes(), k
        again = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
        for k in MARGIN_TABLES:
            assert getattr(again, k).tobytes() == getattr(res, k).tobytes(), k
        # without the decoder's flag the setting does nothing
        bare = f.text_detect(uniform, GROUPED, **WANTS)
        for k in MARGIN_TABLES + ("word_decodes",):
            with pytest.raises(ValueError):
                getattr(bare, k)
        # the moves on
        f.set_word_decode(40, 90)
        moved = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
        check_margins(S, moved, moved.run_costs, moved.words["first_run"], moved.words["n_runs"], table, 40, 90)
        # with the run split the rows are the words' parts, as for the decoder
        split = f.text_detect(uniform, GROUPED, want_word_decode=True, want_run_split=True, **WANTS)
        ws = split.word_splits
        check_margins(S, split, _part_rows(split), ws["first_part"], ws["n_parts"], table, 40, 90)
        never.set_word_decode(40, 90)
        ref = never.text_detect(uniform, GROUPED, want_word_decode=True, want_run_split=True, **WANTS)
        for k in TABLES + DECODE_TABLES + SPLIT_TABLES:
            assert getattr(ref, k).tobytes() == getattr(split, k).tobytes(), k
    finally:
        f.set_word_margin(False)
        f.set_word_decode()
        never.set_word_decode()


def test_setting_off_nothing_is_made_and_nothing_changes(scene):
    S, f, never, prm, path, uniform, table = scene
    f.set_word_margin(True)
    f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
    f.set_word_margin(False)
    for wants in (dict(want_word_decode=True), dict(want_word_decode=True, want_run_split=True)):
        off = f.text_detect(uniform, GROUPED, **wants, **WANTS)
        ref = never.text_detect(uniform, GROUPED, **wants, **WANTS)
        for k in MARGIN_TABLES:
            with pytest.raises(ValueError):
                getattr(off, k)
            with pytest.raises(ValueError):
                getattr(ref, k)
        with pytest.raises(ValueError):
            off.word_decode_margin(0)
        with pytest.raises(ValueError):
            off.word_decode_char_margins(0)
        _same(ref, off)
        for k in TABLES + DECODE_TABLES + (SPLIT_TABLES if "want_run_split" in wants else ()):
            assert getattr(ref, k).tobytes() == getattr(off, k).tobytes(), k


def test_through_a_stream(scene, cascade_paths):
    S, f, never, prm, path, uniform, table = scene
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS | S.WANT_MASKS
    f.set_word_margin(True)
    try:
        res = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
    finally:
        f.set_word_margin(False)
    st = S.FrameStream(prm, depth=2)
    try:
        st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
        st.load_svm_model(path, 1800)
        st.set_bigram(table)
        st.set_word_margin(True)                                         # (on every context of the stream)
        st.submit_copy(uniform, flags, want_run_read=True, want_word_decode=True)
        st.submit_copy(uniform, flags, want_run_read=True, want_word_decode=True)
        for _ in range(2):
            _, a = st.next()
            for k in TABLES + DECODE_TABLES + MARGIN_TABLES:
                assert getattr(a, k).tobytes() == getattr(res, k).tobytes(), k
        st.set_word_margin(False)
        st.submit_copy(uniform, flags, want_run_read=True, want_word_decode=True)
        _, b = st.next()
        with pytest.raises(ValueError):
            b.word_margins
        assert b.word_decodes.tobytes() == res.word_decodes.tobytes()
    finally:
        st.close()
