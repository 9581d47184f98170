"""str_er_set_line_decode in the detect calls, on the frames, the model and the flags of test_word_decode_pipeline.py (two synthetic
text frames of 640 x 480, the size of the sibling pipeline tests: several lines of two and more words): with the setting on the result's
line tables are decode_lines of the same context on the result's own cost rows, gap costs and windows with ==, the gap costs are
line_gap_costs of the returned runs, the windows are the lines' runs, identity (3) of the contract holds against the result's word
decodes, and the accessors agree with the tables; with the setting off the accessors raise and every other table is byte for byte that of
the same call on a context that never had the setting; with STR_ER_WANT_RUN_SPLIT the rows are the words' parts, with (0, 255) between
the parts of one run; on a reused context after a larger call; once through a stream."""
import numpy as np
import pytest

import line_decode_ref as LD
import word_match_ref as WM
from test_frame_lines import GROUPED, _same
from test_run_split_pipeline import _part_rows
from test_svm_exact import _shipped
from test_word_decode_pipeline import DECODE_TABLES
from test_word_match_pipeline import TABLES, WANTS

pytestmark = pytest.mark.gpu
LINE_TABLES = ("line_decodes", "line_decode_chars", "line_decode_src", "line_decode_word_of_row", "line_gap_costs", "line_decode_windows")
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


def check_lines(S, f, res, weight, num=1, den=3, split=False):
    """The line tables of a result against decode_lines of the same context on the result's own rows, gap costs and windows, the gap
    costs against line_gap_costs of the returned runs, identity (3) against the word decodes, and the accessors; returns the number of
    breaks and the number of lines whose segmentation differs from the word gap's.  split: the rows are the words' parts."""
    lw, win, gaps = res.line_words, res.line_decode_windows, res.line_gap_costs
    n_lines = len(res.texts)
    # the rows the decoder read, the run of every row, and the first row and row count of every word
    rows = _part_rows(res) if split else res.run_costs
    row_run = res.split_parts["run"] if split else None
    wfirst, wn = (res.word_splits["first_part"], res.word_splits["n_parts"]) if split else (res.words["first_run"], res.words["n_runs"])
    n_runs = len(rows)
    assert res.line_decodes.dtype == S.LINE_DECODE_DTYPE and len(res.line_decodes) == n_lines == len(lw)
    assert res.line_decode_chars.shape == (3 * n_runs,) and res.line_decode_src.shape == (3 * n_runs,) and res.line_decode_src.dtype == np.uint16
    assert res.line_decode_word_of_row.shape == (n_runs,) and gaps.shape == (n_runs, 2) and win.shape == (n_lines, 2)
    for t in range(n_lines):                             # from the first row of the line's first word to the last row of its last
        ws = range(int(lw[t]["first_word"]), int(lw[t]["first_word"]) + int(lw[t]["n_words"]))
        assert int(win[t, 1]) == sum(int(wn[w]) for w in ws) and (not len(ws) or int(win[t, 0]) == int(wfirst[ws[0]]))
    if not split:
        assert (win[:, 0] == lw["first_run"]).all() and (win[:, 1] == lw["n_runs"]).all()
    assert (gaps == S.line_gap_costs(res.line_runs, win[:, 0], win[:, 1], lw["colmax"], num, den, weight, row_run=row_run)).all()
    assert (gaps == LD.gap_costs([(int(q["x0"]), int(q["x1"])) for q in res.line_runs], win[:, 0], win[:, 1], lw["colmax"], num, den, weight, row_run=row_run)).all()
    if split:                                            # (0, 255) inside a run: a cut is never a blank
        same = np.flatnonzero(row_run[1:] == row_run[:-1]) + 1
        assert (gaps[same] == (0, 255)).all()
    dec, chars, src, wor = f.decode_lines(rows, gaps, win[:, 0], win[:, 1])
    assert res.line_decodes.tobytes() == dec.tobytes() and res.line_decode_chars.tobytes() == chars.tobytes()
    assert res.line_decode_src.tobytes() == src.tobytes() and res.line_decode_word_of_row.tobytes() == wor.tobytes()
    n_breaks = differ = 0
    for t in range(n_lines):
        d, first, m = res.line_decodes[t], int(win[t, 0]), int(win[t, 1])
        words = range(int(lw[t]["first_word"]), int(lw[t]["first_word"]) + int(lw[t]["n_words"]))
        if int(d["cost"]) < 0:
            assert m > 1024
            continue
        # (3) the word gap's segmentation is one path: never worse than its words' decodes with what it pays at its gaps
        if all(int(res.word_decodes[w]["cost"]) >= 0 for w in words):
            starts = {int(wfirst[w]) for w in words}
            paid = sum(int(gaps[r, 1]) if r in starts else int(gaps[r, 0]) for r in range(first + 1, first + m))
            assert int(d["cost"]) <= sum(int(res.word_decodes[w]["cost"]) for w in words) + paid, t
        text, parts = res.line_decode_text(t), res.line_decode_words(t)
        assert text.count(" ") == int(d["n_breaks"]) == len(parts) - 1 and " ".join(p[0] for p in parts) == text
        assert len(text) == int(d["n_chars"])
        for s, box in parts:
            assert (box is None or (box[2] > 0 and box[3] > 0)) and (s != "" or box is None)
        n_breaks += int(d["n_breaks"])
        word_of = res.line_decode_word_of_row[first:first + m]
        gap_word = np.concatenate([np.full(int(wn[w]), k) for k, w in enumerate(words)]) if m else np.zeros(0, np.int64)
        differ += int(not ((word_of == gap_word) | (word_of < 0)).all())
    for i in range(len(res.frame_lines)):
        assert res.frame_line_line_decode_text(i) == res.line_decode_text(int(res.frame_lines[i]["rep"]))
    return n_breaks, differ


def test_setting_on_the_lines_are_decode_lines_on_the_result_s_rows(scene):
    S, f, never, prm, path, uniform, table = scene
    f.set_line_decode(True)                              # (the default weight, 16)
    try:
        res = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
        assert int((res.line_words["n_words"] >= 2).sum()) >= 2 and len(res.words) > 10
        n_breaks, differ = check_lines(S, f, res, 16)
        assert n_breaks > 0
        # everything else is the call of a context that never had the setting
        ref = never.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
        _same(ref, res)
        for k in TABLES + DECODE_TABLES:
            assert getattr(ref, k).tobytes() == getattr(res, k).tobytes(), k
        again = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
        for k in LINE_TABLES:
            assert getattr(again, k).tobytes() == getattr(res, k).tobytes(), k
        # without the decoder's flag the setting does nothing
        bare = f.text_detect(uniform, GROUPED, **WANTS)
        for k in LINE_TABLES + ("word_decodes",):
            with pytest.raises(ValueError):
                getattr(bare, k)
        # the moves on, another weight, another word gap: the table alone decides at weight 0
        f.set_word_decode(40, 90)
        f.set_line_decode(True, 0)
        moved = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
        check_lines(S, f, moved, 0)
        assert (moved.line_gap_costs[:, 0] == 0).all()
        f.set_line_decode(True, 127)
        f.set_word_gap(2, 3)
        heavy = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
        check_lines(S, f, heavy, 127, 2, 3)
        assert int(heavy.line_gap_costs[:, 1][heavy.line_gap_costs[:, 1] < 255].max()) > 127
    finally:
        f.set_line_decode(False)
        f.set_word_decode()
        f.set_word_gap(1, 3)


def test_setting_off_nothing_is_made_and_nothing_changes(scene):
    S, f, never, prm, path, uniform, table = scene
    f.set_line_decode(True)
    f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
    f.set_line_decode(False)
    for wants in (dict(want_word_decode=True), dict(want_word_decode=True, want_run_split=True)):
        off = f.text_detect(uniform, GROUPED, **wants, **WANTS)
        ref = never.text_detect(uniform, GROUPED, **wants, **WANTS)
        for k in LINE_TABLES:
            with pytest.raises(ValueError):
                getattr(off, k)
            with pytest.raises(ValueError):
                getattr(ref, k)
        with pytest.raises(ValueError):
            off.line_decode_text(0)
        _same(ref, off)
        for k in TABLES + DECODE_TABLES + (SPLIT_TABLES if "want_run_split" in wants else ()):
            assert getattr(ref, k).tobytes() == getattr(off, k).tobytes(), k


def test_with_the_run_split_the_rows_are_the_parts(scene):
    S, f, never, prm, path, uniform, table = scene
    f.set_line_decode(True)
    try:
        for ins, dele in ((0, 0), (40, 90)):
            f.set_word_decode(ins, dele)
            never.set_word_decode(ins, dele)
            split = f.text_detect(uniform, GROUPED, want_word_decode=True, want_run_split=True, **WANTS)
            assert len(split.split_parts) >= len(split.line_runs) > 0
            check_lines(S, f, split, 16, split=True)
            ref = never.text_detect(uniform, GROUPED, want_word_decode=True, want_run_split=True, **WANTS)
            _same(ref, split)
            for k in TABLES + DECODE_TABLES + SPLIT_TABLES:
                assert getattr(ref, k).tobytes() == getattr(split, k).tobytes(), k
            again = f.text_detect(uniform, GROUPED, want_word_decode=True, want_run_split=True, **WANTS)
            for k in LINE_TABLES:
                assert getattr(again, k).tobytes() == getattr(split, k).tobytes(), k
        bare = f.text_detect(uniform, GROUPED, want_run_split=True, **WANTS)       # (without the decoder's flag the setting does nothing)
        with pytest.raises(ValueError):
            bare.line_decodes
        check_lines(S, f, f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS), 16)
    finally:
        f.set_line_decode(False)
        f.set_word_decode()
        never.set_word_decode()


def test_on_a_reused_context_after_a_larger_call(scene, cascade_paths):
    S, f, never, prm, path, uniform, table = scene
    f.set_line_decode(True)
    try:
        big = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
        grown = f.line_decode_stats()["table_bytes"]
        assert grown >= 68 * 2 * len(big.line_runs)
        small = f.text_detect(uniform[1:], GROUPED, want_word_decode=True, **WANTS)
        assert 0 < len(small.line_runs) < len(big.line_runs) and f.line_decode_stats()["table_bytes"] == grown
        check_lines(S, f, small, 16)
        fresh = S.ERFilter(params=prm)
        try:
            fresh.load_cascade(0, cascade_paths[0]); fresh.load_cascade(1, cascade_paths[1])
            fresh.load_svm_model(path, 1800)
            fresh.set_bigram(table)
            fresh.set_line_decode(True)
            ref = fresh.text_detect(uniform[1:], GROUPED, want_word_decode=True, **WANTS)
            for k in LINE_TABLES + DECODE_TABLES:
                assert getattr(ref, k).tobytes() == getattr(small, k).tobytes(), k
        finally:
            fresh.close()
        check_lines(S, f, f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS), 16)
    finally:
        f.set_line_decode(False)


def test_through_a_stream(scene, cascade_paths):
    S, f, never, prm, path, uniform, table = scene
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS | S.WANT_MASKS
    f.set_line_decode(True, 24)
    try:
        res = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
    finally:
        f.set_line_decode(False)
    st = S.FrameStream(prm, depth=2)
    try:
        st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
        st.load_svm_model(path, 1800)
        st.set_bigram(table)
        st.set_line_decode(True, 24)                                     # (on every context of the stream)
        st.submit_copy(uniform, flags, want_run_read=True, want_word_decode=True)
        st.submit_copy(uniform, flags, want_run_read=True, want_word_decode=True)
        for _ in range(2):
            _, a = st.next()
            for k in TABLES + DECODE_TABLES + LINE_TABLES:
                assert getattr(a, k).tobytes() == getattr(res, k).tobytes(), k
        st.set_line_decode(False)
        st.submit_copy(uniform, flags, want_run_read=True, want_word_decode=True)
        _, b = st.next()
        with pytest.raises(ValueError):
            b.line_decodes
        assert b.word_decodes.tobytes() == res.word_decodes.tobytes()
    finally:
        st.close()
