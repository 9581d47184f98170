"""str_er_set_line_lattice_decode in the detect calls, on the scene and the context of test_lattice_decode_pipeline.py (the S-text frames
of seeds 2 and 976, two pyramid levels, read with a model made from the frame call's own pieces, so that words split; a bigram table of
the words it reads, INS / DEL on): with the setting on the result's tables are exactly what str_er_lattice_decode_lines_host gives on the
result's own split records, rows, gap costs and windows, the gap costs are line_gap_costs of the returned runs, the windows are the
lines' runs, and the accessors agree with the tables; with the setting off the accessors raise, the back-pointer table is never made,
and every other table -- the line decode's on the split parts included -- is byte for byte the same with the setting on and off."""
import numpy as np
import pytest

import line_decode_ref as LD
import line_lattice_ref as LL
from test_frame_lines import GROUPED
from test_lattice_decode_pipeline import DEL, INS, LATTICE_TABLES, SPLITS, proto  # noqa: F401  (the fixture)
from test_line_decode_pipeline import LINE_TABLES
from test_run_split_pipeline import SPLIT, SPLIT_TABLES, scene  # noqa: F401  (the fixture's fixture)
from test_word_decode_pipeline import DECODE_TABLES
from test_word_match_pipeline import TABLES

pytestmark = pytest.mark.gpu
LL_TABLES = ("line_lattice_decodes", "line_lattice_chars", "line_lattice_src", "line_lattice_parts", "line_lattice_word_of_part", "line_lattice_gap_costs",
             "line_lattice_windows")


def check_lines(S, g, res, table, weight, num=1, den=3):
    """The setting's tables against the host entry point on the result's own rows, gap costs and windows, the GPU twin, the gap costs
    against line_gap_costs of the returned runs and the accessors; returns (breaks, parts that are pieces)."""
    lw, win, gaps = res.line_words, res.line_lattice_windows, res.line_lattice_gap_costs
    n_lines, n_runs = len(res.texts), len(res.line_runs)
    atoms = int((res.run_splits["n_cuts"] + 1).sum())
    d = res.line_lattice_decodes
    assert d.dtype == S.LINE_LATTICE_DECODE_DTYPE and len(d) == n_lines == len(lw) and win.shape == (n_lines, 2) and gaps.shape == (n_runs, 2)
    assert res.line_lattice_chars.shape == (3 * atoms,) and res.line_lattice_src.shape == (3 * atoms,) and res.line_lattice_src.dtype == np.uint16
    assert res.line_lattice_parts.dtype == S.SPLIT_PART_DTYPE and len(res.line_lattice_parts) == len(res.line_lattice_word_of_part) == int(d["n_parts"].sum())
    # a window: from the first run of the line's first word to the last run of its last
    assert (win[:, 0] == lw["first_run"]).all() and (win[:, 1] == lw["n_runs"]).all()
    for t in range(n_lines):
        ws = range(int(lw[t]["first_word"]), int(lw[t]["first_word"]) + int(lw[t]["n_words"]))
        assert int(win[t, 1]) == sum(int(res.words[w]["n_runs"]) for w in ws) and (not len(ws) or int(win[t, 0]) == int(res.words[ws[0]]["first_run"]))
    assert (gaps == S.line_gap_costs(res.line_runs, win[:, 0], win[:, 1], lw["colmax"], num, den, weight)).all()
    assert (gaps == LD.gap_costs([(int(q["x0"]), int(q["x1"])) for q in res.line_runs], win[:, 0], win[:, 1], lw["colmax"], num, den, weight)).all()
    got = (d, res.line_lattice_chars, res.line_lattice_src, res.line_lattice_parts, res.line_lattice_word_of_part)
    host = S.lattice_decode_lines_host(res.run_splits, res.run_costs, res.piece_costs, gaps, win[:, 0], win[:, 1], table, INS, DEL, SPLIT)
    twin = g.lattice_decode_lines(res.run_splits, res.run_costs, res.piece_costs, gaps, win[:, 0], win[:, 1])
    for k, (a, h, w) in enumerate(zip(got, host, twin)):
        assert a.tobytes() == h.tobytes() == w.tobytes(), LL_TABLES[k]
    assert d["first_part"].tolist() == np.concatenate([[0], np.cumsum(d["n_parts"])])[:-1].tolist()
    assert (d["n_sub"] + d["n_ins"] + d["n_breaks"] == d["n_chars"]).all() and (d["n_sub"] + d["n_del"] == d["n_parts"]).all()
    slot = LL.node_slots(res.run_splits)
    for t in range(n_lines):
        if int(d[t]["cost"]) < 0:
            assert int(win[t, 1]) > 1024
            continue
        N = int(slot[win[t, 0] + win[t, 1]] - slot[win[t, 0]])
        assert int(win[t, 1]) <= int(d[t]["n_parts"]) <= N
        text, words = res.line_lattice_text(t), res.line_lattice_words(t)
        assert text.count(" ") == int(d[t]["n_breaks"]) == len(words) - 1 and " ".join(w[0] for w in words) == text and len(text) == int(d[t]["n_chars"])
        for s, parts, box in words:
            assert (box is None or (box[2] > 0 and box[3] > 0)) and (s != "" or box is None)
            assert ((parts["run"] >= win[t, 0]) & (parts["run"] < win[t, 0] + win[t, 1])).all()
    for i in range(len(res.frame_lines)):
        assert res.frame_line_line_lattice_text(i) == res.line_lattice_text(int(res.frame_lines[i]["rep"]))
    n_breaks, n_pieces = int(d["n_breaks"].sum()), int((res.line_lattice_parts["piece"] >= 0).sum())
    print(f"{n_lines} lines, {n_runs} runs, {atoms} atoms, {len(res.line_lattice_parts)} parts of which {n_pieces} pieces, {n_breaks} breaks at weight {weight}")
    return n_breaks, n_pieces


def test_setting_on_the_tables_are_the_host_s_on_the_result_s_own_rows(proto):  # noqa: F811
    S, g, prm, model, uniform, crops, base, base_crops, table, read = proto
    # the setting off: a call with the lattice decode makes none of the setting's tables and no back-pointer table
    off = g.text_detect(uniform, GROUPED, want_lattice_decode=True, **SPLITS)
    for k in LL_TABLES:
        with pytest.raises(ValueError):
            getattr(off, k)
    assert g.line_lattice_decode_stats()["table_bytes"] == 0
    g.set_line_lattice_decode(True)                       # (the default weight, 16)
    try:
        bare = g.text_detect(uniform, GROUPED, **SPLITS)     # without the lattice decode's flag the setting does nothing
        for k in LL_TABLES:
            with pytest.raises(ValueError):
                getattr(bare, k)
        assert g.line_lattice_decode_stats()["table_bytes"] == 0
        res = g.text_detect(uniform, GROUPED, want_lattice_decode=True, **SPLITS)
        n_breaks, n_pieces = check_lines(S, g, res, table, 16)
        assert n_pieces >= 1 and n_breaks >= 1              # the condition: some decoded part is a piece, and some line breaks
        assert g.line_lattice_decode_stats()["table_bytes"] >= 4 * 68 * int((res.run_splits["n_cuts"] + 1).sum())
        for k in TABLES + SPLIT_TABLES + LATTICE_TABLES:     # every other table is that of the call with the setting off
            assert getattr(off, k).tobytes() == getattr(res, k).tobytes(), k
        again = g.text_detect(uniform, GROUPED, want_lattice_decode=True, **SPLITS)
        for k in LL_TABLES:
            assert getattr(again, k).tobytes() == getattr(res, k).tobytes(), k
        # another weight and the table alone (weight 0)
        for weight in (0, 127):
            g.set_line_lattice_decode(True, weight)
            check_lines(S, g, g.text_detect(uniform, GROUPED, want_lattice_decode=True, **SPLITS), table, weight)
        g.set_line_lattice_decode(True)
        # the list call
        lst = g.text_detect_list(crops, GROUPED, want_lattice_decode=True, **SPLITS)
        check_lines(S, g, lst, table, 16)
        for k in TABLES + SPLIT_TABLES:
            assert getattr(base_crops, k).tobytes() == getattr(lst, k).tobytes(), k
    finally:
        g.set_line_lattice_decode(False)


def test_beside_the_decoder_and_the_line_decode_on_the_split_parts(proto):  # noqa: F811
    """With the word decoder and the line decode on the split parts (its second wait) in the same call: their tables, and every other
    table, are byte for byte the same with this setting on and off, and this setting's are those of the call without them."""
    S, g, prm, model, uniform, crops, base, base_crops, table, read = proto
    g.set_line_decode(True)
    try:
        off = g.text_detect(uniform, GROUPED, want_lattice_decode=True, want_word_decode=True, **SPLITS)
        g.set_line_lattice_decode(True)
        on = g.text_detect(uniform, GROUPED, want_lattice_decode=True, want_word_decode=True, **SPLITS)
        for k in TABLES + SPLIT_TABLES + LATTICE_TABLES + DECODE_TABLES + LINE_TABLES:
            assert getattr(off, k).tobytes() == getattr(on, k).tobytes(), k
        g.set_line_decode(False)
        alone = g.text_detect(uniform, GROUPED, want_lattice_decode=True, **SPLITS)
        for k in LL_TABLES:
            assert getattr(alone, k).tobytes() == getattr(on, k).tobytes(), k
        check_lines(S, g, on, table, 16)
    finally:
        g.set_line_decode(False)
        g.set_line_lattice_decode(False)
