"""str_er_set_line_margin in the detect calls, on the call of test_line_decode_pipeline.py (two synthetic text frames of 640 x 480, two
pyramid levels, the shipped model): with the setting on every margin table equals line_margins_host on the result's own rows, windows
and gap costs with ==, without STR_ER_WANT_RUN_SPLIT and with it (then the rows are the words' parts, behind a row map, which nothing
else reaches); with the setting off no accessor returns a table and every other table is byte for byte that of the same call on a
context that never had the setting."""
import numpy as np
import pytest

import word_match_ref as WM
from test_frame_lines import GROUPED, _same
from test_line_decode_pipeline import LINE_TABLES, SPLIT_TABLES
from test_run_split_pipeline import _part_rows
from test_svm_exact import _shipped
from test_word_decode_pipeline import DECODE_TABLES
from test_word_match_pipeline import TABLES, WANTS

pytestmark = pytest.mark.gpu
MARGIN_TABLES = ("line_margins", "line_row_margins", "line_row_reads", "line_row_alts", "line_gap_margins", "line_gap_moves")


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
        f.set_line_decode(True)
    yield S, pair[0], pair[1], uniform, table
    for f in pair:
        f.close()


def check_margins(S, res, table, ins, dele, split=False):
    """The margin tables of a result against line_margins_host on the result's own rows, gap costs and windows, and the accessors;
    returns the number of gaps with an alternative."""
    rows = _part_rows(res) if split else res.run_costs
    win, n = res.line_decode_windows, len(rows)
    want = S.line_margins_host(rows, res.line_gap_costs, win[:, 0], win[:, 1], table, ins, dele)
    assert res.line_margins.dtype == S.LINE_MARGIN_DTYPE and len(res.line_margins) == len(res.texts)
    assert res.line_row_margins.shape == (n,) and res.line_row_margins.dtype == np.int32 and res.line_gap_moves.shape == (n,)
    for k, b in zip(MARGIN_TABLES, want):
        a = getattr(res, k)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    for t in range(len(res.texts)):
        first, m = int(win[t, 0]), int(win[t, 1])
        assert res.line_decode_margin(t) == int(res.line_margins[t]["margin"])
        gaps = res.line_break_margins(t)
        assert len(gaps) == max(0, m - 1) and all(res.line_gap_moves[first + k] == mv and res.line_gap_margins[first + k] == g for k, mv, g in gaps)
        if m:                                            # the moves are the decoded string's breaks, the readings its characters
            d = res.line_decodes[t]
            assert int((res.line_gap_moves[first:first + m] == 1).sum()) == int(d["n_breaks"])
            assert int((res.line_row_reads[first:first + m] == 65).sum()) == int(d["n_del"])
    return int((res.line_gap_margins >= 0).sum())


def test_setting_off_nothing_is_made_and_nothing_changes(scene):
    S, f, never, uniform, table = scene
    f.set_line_margin(True)
    f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
    f.set_line_margin(False)
    for wants in (dict(want_word_decode=True), dict(want_word_decode=True, want_run_split=True)):
        off = f.text_detect(uniform, GROUPED, **wants, **WANTS)
        ref = never.text_detect(uniform, GROUPED, **wants, **WANTS)
        for k in MARGIN_TABLES:
            with pytest.raises(ValueError):
                getattr(off, k)
            with pytest.raises(ValueError):
                getattr(ref, k)
        with pytest.raises(ValueError):
            off.line_decode_margin(0)
        _same(ref, off)
        for k in TABLES + DECODE_TABLES + LINE_TABLES + (SPLIT_TABLES if "want_run_split" in wants else ()):
            assert getattr(ref, k).tobytes() == getattr(off, k).tobytes(), k
    assert never.line_margin_stats()["table_bytes"] == 0 and f.line_margin_stats()["table_bytes"] > 0      # (off: nothing is allocated)


def test_setting_on_the_margins_are_the_host_s_on_the_result_s_rows(scene):
    S, f, never, uniform, table = scene
    f.set_line_margin(True)
    try:
        for ins, dele in ((0, 0), (40, 90)):
            f.set_word_decode(ins, dele)
            never.set_word_decode(ins, dele)
            res = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
            assert int((res.line_words["n_words"] >= 2).sum()) >= 2 and len(res.words) > 10
            assert check_margins(S, res, table, ins, dele) > 0
            assert f.line_margin_stats()["table_bytes"] >= 544 * len(res.line_runs)
            # everything else is the call of a context that never had the setting
            ref = never.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
            _same(ref, res)
            for k in TABLES + DECODE_TABLES + LINE_TABLES:
                assert getattr(ref, k).tobytes() == getattr(res, k).tobytes(), k
            again = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
            for k in MARGIN_TABLES:
                assert getattr(again, k).tobytes() == getattr(res, k).tobytes(), k
        # without the decoder's flag, or without the line decode, the setting does nothing
        bare = f.text_detect(uniform, GROUPED, **WANTS)
        f.set_line_decode(False)
        no_lines = f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS)
        f.set_line_decode(True)
        for k in MARGIN_TABLES:
            with pytest.raises(ValueError):
                getattr(bare, k)
            with pytest.raises(ValueError):
                getattr(no_lines, k)
    finally:
        f.set_line_margin(False)
        f.set_word_decode()
        never.set_word_decode()


def test_with_the_run_split_the_rows_are_the_parts(scene):
    S, f, never, uniform, table = scene
    f.set_line_margin(True)
    try:
        for ins, dele in ((0, 0), (40, 90)):
            f.set_word_decode(ins, dele)
            never.set_word_decode(ins, dele)
            split = f.text_detect(uniform, GROUPED, want_word_decode=True, want_run_split=True, **WANTS)
            assert len(split.split_parts) >= len(split.line_runs) > 0
            assert check_margins(S, split, table, ins, dele, split=True) > 0
            ref = never.text_detect(uniform, GROUPED, want_word_decode=True, want_run_split=True, **WANTS)
            _same(ref, split)
            for k in TABLES + DECODE_TABLES + LINE_TABLES + SPLIT_TABLES:
                assert getattr(ref, k).tobytes() == getattr(split, k).tobytes(), k
        # and back on the runs' rows, on the same context
        f.set_word_decode()
        check_margins(S, f.text_detect(uniform, GROUPED, want_word_decode=True, **WANTS), table, 0, 0)
    finally:
        f.set_line_margin(False)
        f.set_word_decode()
        never.set_word_decode()
