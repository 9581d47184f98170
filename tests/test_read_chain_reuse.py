"""The reading chain on a reused context: feet_words, feet_read, feet_split, split_words, match_words, decode_words, lattice_decode_words,
lattice_match_words, match_tracks, lattice_match_tracks, decode_tracks, word_margins, lattice_margins, lattice_decode_tracks, decode_lines,
line_margins and two track pools run on ONE context on a small input, a large one, the small one again, both again with the entry
points in reverse order, and under a lexicon of several chunks that is swapped in and out -- so that every call finds in its on-demand
buffers (wm_tab, wd_tab, wg_tab, rs_tab, rs_out, ld_tab, lg_tab, lm_tab, tm_tab, lt_tab, td_tab, ltd_tab, ln_tab, ln_bp, ln_fw, run_tab,
run_atlas, the pools' rows / tab) the records of a call with another layout.  The small input (read_chain_cases.py) consists of
the records a kernel or a fill writes as constants, the large one has a live record in every slot: a slot nobody writes shows as a
stale record.  Every output equals the host entry point's on the same input byte for byte (feet_words: line_words_ref.py; feet_read
and feet_split, which have no host twin: the same call on a brand-new context, and once their modules' references), every small round
equals the first, the buffers grow once and workspace_bytes() never.  Then the fused detect call with the five settings on
(set_word_margin, set_lattice_margin, set_lattice_track_decode, set_line_decode, set_line_margin), a blank frame, a list call and the
single-stage rounds take turns on one context (read_rows, the shared scratch, ln_bp and ln_fw change hands).  test_on_demand_buffers.py does the
same for the buffers up to feet_geom.

What was tried against it, each edit only leaving out a write of default values: without the 0xFF fill of member_cost in
track_match_enqueue the member slots of no track hold 0 on a fresh buffer and a larger call's member indices on a reused one (round 1 and
every small round after a large one fail against match_tracks_host); the same fill in track_decode_enqueue likewise.  The loop that writes
-1 for the members of an undecoded track in k_track_decode cannot be seen by any test: that fill has written the same slots on the same
stream before the launch.  Without both, the slots of the tracks of unusable members and of no seeds are stale as well.

The five newer stages, one library build for each edit, all rounds run until the first failure:
  decode_lines, line_margins   without the 0xFF preset of the line tables in line_decode_enqueue the labels of the rows of no line are not
                               0xFF: round 1 fails at decode_lines (the label bytes from 3 * 1025 on, against decode_lines_host).
                               Without the loops of k_line_decode that write 0xFF / 0xFFFF / -1 over a line of more than 1024 rows, and
                               without the loops and the record of -1 that k_line_margin writes for a line without rows or of more than 1024
                               rows, every round passes: no test can see them, that preset has written the same bytes into the same slots on
                               the same stream before the launch (the records of the margins lie in the preset too).
  word_margins                 without the stores of the record and the rows of a word that is not decoded (0 or 33 runs), and of the rows
                               a decoded word does not have, in k_word_margin: round 1 fails at word_margins, records 0 and 1.
  lattice_margins              the same stores of k_lattice_margin for a word of no runs or of an unusable lattice: round 1 fails at
                               lattice_margins, records 0, 1 and 2.
  lattice_decode_tracks        without the member record and the 0xFF sources that k_lattice_track_decode_members writes for a slot of no
                               track: round 1 fails at the member records 0, 1, 4, 5, 8 ...; without the record and the 0xFF labels of a track
                               without seeds in the track kernel (n_used kept): round 1 fails at the track records 0, 1, 3, 4.
A fresh buffer holds zeros and these defaults are -1 and 0xFF, so each of them shows in round 1 already; the small rounds behind a large
one hold the same slots against a larger call's records.

The first section needs no GPU: it proves on the host entry points that the cases are what they claim to be."""
import numpy as np
import pytest

import line_words_ref as LW
import read_chain_cases as RC
import run_read_ref as RR
import run_split_ref as RS
import track_decode_ref as TD
from test_frame_lines import GROUPED
from test_lattice_decode_pipeline import INS as DEC_INS, DEL as DEC_DEL, LATTICE_TABLES, proto  # noqa: F401  (the fixture)
from test_lattice_margin_pipeline import MARGIN_TABLES as LATTICE_MARGIN_TABLES
from test_lattice_match_pipeline import BAND, DEL, INS, MATCH_TABLES, OTHER_TABLES, lex  # noqa: F401  (the fixture)
from test_lattice_track_decode_pipeline import NEW as LATTICE_TRACK_DECODE_TABLES
from test_lattice_track_pipeline import READ_TABLES, TRACK_TABLES
from test_line_decode_pipeline import LINE_TABLES
from test_line_margin_pipeline import MARGIN_TABLES as LINE_MARGIN_TABLES
from test_line_words import _feet
from test_read_chain_combos import DECODE_TABLES
from test_run_split_pipeline import DEN, NUM, SPLIT, scene  # noqa: F401  (the fixture lex builds on)
from test_svm_exact import _shipped
from test_track_decode_pipeline import NEW as TRACK_DECODE_TABLES
from test_track_pool import EMPTY as POOL_EMPTY, reference as pool_reference
from test_word_margin_pipeline import MARGIN_TABLES as WORD_MARGIN_TABLES

STAGES = ("feet_words", "feet_read", "feet_split", "split_words", "match_words", "decode_words", "lattice_decode_words", "lattice_match_words",
          "match_tracks", "lattice_match_tracks", "decode_tracks", "word_margins", "lattice_margins", "lattice_decode_tracks", "decode_lines", "line_margins")
FEET_STAGES = STAGES[:3]
SPLIT_KEYS = ("line_words", "runs", "words", "reads", "q", "splits", "pieces", "piece_reads", "piece_q")
NO_MATCH = (-1, -1, -1, -1)
NO_MARGIN, NO_LATTICE_MARGIN, NO_LINE_MARGIN = (-1,) * 4, (-1,) * 7 + (0,), (-1,) * 8
NO_LINE = (-1, 0, 0, 0, 0, 0)
NO_MEMBER = (-1, 0, 0, 0)               # (cost, n_parts, n_del, n_ins of a member that took no part; first_part is where the parts stand, word the slot's)
DEFAULTS = dict(fold=True, ins=64, dele=64, band=2, num=1, den=4, split=8, dec_ins=0, dec_dele=0, td_ins=64, td_dele=64, rounds=8)
# every table a result of the fused call exposes
FUSED = dict(want_masks=True, want_frame_lines=True, want_line_links=True, want_line_words=True, want_run_read=True, want_word_match=True, want_word_decode=True,
             want_run_split=True, want_track_read=True, want_lattice_decode=True, want_lattice_match=True, want_lattice_track=True, want_track_decode=True)
assert OTHER_TABLES[:5] == ("line_words", "line_runs", "words", "run_reads", "run_features") and OTHER_TABLES[11] == "run_splits" and READ_TABLES[5] == "track_member_costs"
SETTING_TABLES = WORD_MARGIN_TABLES + LATTICE_MARGIN_TABLES + LATTICE_TRACK_DECODE_TABLES + LINE_TABLES + LINE_MARGIN_TABLES          # the five settings'
READING_TABLES = tuple(dict.fromkeys(OTHER_TABLES[:5] + OTHER_TABLES[11:] + DECODE_TABLES + LATTICE_TABLES + MATCH_TABLES + READ_TABLES[:6] + TRACK_TABLES + TRACK_DECODE_TABLES
                                     + SETTING_TABLES))
FUSED_TABLES = tuple(dict.fromkeys(OTHER_TABLES + READ_TABLES + READING_TABLES))


# ---- the cases and their host references, made once ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cases(S):
    """{size: {feet, ft, bits, rows, td, lines}} and the lexicons and the table."""
    out = {"lex": dict(zip(("one", "big"), RC.lexicons())), "B": RC.bigram()}
    for size in RC.SIZES:
        feet = RC.feet_case(size)
        ft, bits = _feet(S, feet["items"])
        rows = RC.rows_case(S, size)
        out[size] = {"feet": feet, "ft": ft, "bits": bits, "rows": rows, "td": RC.track_decode_case(size), "lines": RC.lines_case(rows, size)}
    return out


def _args(c):
    r = c["rows"]
    return (r["rc"], r["first"], r["n_of"]), (r["sp"], r["rc"], r["pc"], r["first"], r["n_of"]), (r["tf"], r["tc"], r["mem"])


def _lines(c):
    L = c["lines"]
    return L["costs"], L["gaps"], L["first"], L["n_of"]


def host_round(S, c, words, B, p=DEFAULTS):
    """The host entry points on a case under the lexicon `words`, the table B and the settings p: {stage: tuple of arrays}."""
    rows, lat, tr = _args(c)
    return {"split_words": S.split_words_host(*lat, p["split"]),
            "match_words": (S.match_words_host(*rows, words, p["fold"], p["ins"], p["dele"], p["band"]),),
            "decode_words": S.decode_words_host(*rows, B, p["dec_ins"], p["dec_dele"]),
            "lattice_decode_words": S.lattice_decode_words_host(*lat, B, p["dec_ins"], p["dec_dele"], p["split"]),
            "lattice_match_words": S.lattice_match_words_host(*lat, words, p["fold"], p["ins"], p["dele"], p["band"], p["split"]),
            "match_tracks": S.match_tracks_host(*rows, *tr, words, p["fold"], p["ins"], p["dele"], p["band"]),
            "lattice_match_tracks": S.lattice_match_tracks_host(*lat, *tr, words, p["fold"], p["ins"], p["dele"], p["band"], p["split"]),
            "decode_tracks": S.decode_tracks_host(*c["td"]["packed"], B, p["dec_ins"], p["dec_dele"], p["td_ins"], p["td_dele"], p["rounds"]),
            "word_margins": S.word_margins_host(*rows, B, p["dec_ins"], p["dec_dele"])[:4],
            "lattice_margins": S.lattice_margins_host(*lat, B, p["dec_ins"], p["dec_dele"], p["split"])[:6],
            "lattice_decode_tracks": S.lattice_decode_tracks_host(*lat, *c["rows"]["ltd"], B, p["dec_ins"], p["dec_dele"], p["td_ins"], p["td_dele"], p["rounds"], p["split"]),
            "decode_lines": S.decode_lines_host(*_lines(c), B, p["dec_ins"], p["dec_dele"]),
            "line_margins": S.line_margins_host(*_lines(c), B, p["dec_ins"], p["dec_dele"])}


@pytest.fixture(scope="module")
def host(S, cases):
    """host_round of both sizes under both lexicons at the default settings, each made when it is first asked for."""
    made = {}

    def get(size, name):
        if (size, name) not in made:
            made[size, name] = host_round(S, cases[size], cases["lex"][name], cases["B"])
        return made[size, name]
    return get


def tuples(rec):
    return [tuple(int(v) for v in r) for r in rec.tolist()]


# ---- 1. the cases are what they claim to be (no GPU) ---------------------------------------------------------------------------------------

def test_the_lexicons_have_one_and_several_chunks(cases):
    assert RC.chunks(cases["lex"]["one"]) == (1, 1)
    tm, wm = RC.chunks(cases["lex"]["big"])
    assert 4900 <= len(cases["lex"]["big"]) <= 5100 and tm >= 4 and wm >= 2
    assert len({len(w) for w in cases["lex"]["big"]}) >= 10


def test_the_large_case_is_16_times_the_small_one(cases, host):
    small, large = cases["small"], cases["large"]
    for key in ("first", "mem"):                               # words, member slots
        assert len(large["rows"][key]) >= 16 * len(small["rows"][key]), key
    for key, at in (("first", 1), ("mem", 5)):                 # ... and those of the track decode
        assert len(large["td"]["packed"][at]) >= 16 * len(small["td"]["packed"][at]), key
    assert len(large["feet"]["items"]) >= 16 * len(small["feet"]["items"])
    for name in ("one", "big"):
        hs, hl = host("small", name), host("large", name)
        for stage, at in (("split_words", 1), ("lattice_decode_words", 3), ("lattice_match_words", 2), ("lattice_match_tracks", 3)):          # part slots
            assert len(hl[stage][at]) >= 16 * max(1, len(hs[stage][at])), (name, stage)
    hs, hl = host("small", "one"), host("large", "one")
    for stage in STAGES[11:]:                                  # every table of the five newer stages: words, tracks, member slots, parts, lines, rows
        for at, (a, b) in enumerate(zip(hs[stage], hl[stage])):
            assert len(b) >= 16 * max(1, len(a)), (stage, at)


@pytest.mark.parametrize("name", ["one", "big"])
def test_the_small_case_is_the_constant_records(cases, host, name):
    """Which records of `small` are the empty record and which member costs are -1: what round 3 spells out on the GPU."""
    h, r = host("small", name), cases["small"]["rows"]
    runs = [len(c) for c in r["shapes"]]
    nodes = [sum(k + 1 for k in c) for c in r["shapes"]]
    assert runs == [0, 33, 9, 4, 3] and nodes == [0, 33, 36, 7, 4]
    mw = tuples(h["match_words"][0])
    assert [m[:4] == NO_MATCH and m[5] == 0 for m in mw] == [False, True, False, False, False]
    lm = tuples(h["lattice_match_words"][0])
    assert [m[:4] == NO_MATCH and m[5] == 0 and m[7:] == (0, 0, 0) for m in lm] == [False, True, True, False, False]
    assert lm[0][7] == 0 and lm[3][7] >= 4 and lm[4][7] >= 3          # a word of no runs has no parts either; the ordinary ones have
    assert (h["lattice_match_words"][1][[1, 2]] == 255).all()
    sw = tuples(h["split_words"][0])
    assert sw[0] == (0, 0, 0, 0) and [w[1] >= n for w, n in zip(sw[1:], runs[1:])] == [True] * 4
    dw, ld = tuples(h["decode_words"][0]), tuples(h["lattice_decode_words"][0])
    B = cases["B"]
    assert [d[0] for d in dw] == [int(B[65, 65]), -1, dw[2][0], dw[3][0], dw[4][0]] and min(dw[2][0], dw[3][0], dw[4][0]) >= 0
    assert [d[0] == -1 for d in ld] == [False, True, True, False, False] and [d[7] for d in ld] == [0, 0, 0, ld[3][7], ld[4][7]] and ld[3][7] >= 4 and ld[4][7] >= 3
    assert (h["lattice_decode_words"][1][[1, 2]] == 255).all()
    # the tracks: none, unusable members only, ordinary, usable by the rows alone; GAP slots of no track behind each
    assert r["tracks"] == [[], [1, 1], [3, 4], [2, 2]] and r["tf"].tolist() == [0, 2, 6, 10] and len(r["mem"]) == 14
    in_track = [2, 3, 6, 7, 10, 11]
    free = [i for i in range(14) if i not in in_track]
    mt, mc = tuples(h["match_tracks"][0]), h["match_tracks"][1].tolist()
    assert mt[0] == NO_MATCH + (0, 0, 0, -1) and mt[1][:4] == NO_MATCH and mt[1][4] > 0 and mt[1][5:] == (0, 0, -1) and mt[2][0] >= 0 and mt[3][0] >= 0
    assert [i for i in range(14) if mc[i] == -1] == sorted(free + [2, 3])
    lt, lmem, lsrc, lparts = h["lattice_match_tracks"]
    lt, lmem = tuples(lt), tuples(lmem)
    assert lt[0] == mt[0] and lt[1] == mt[1] and lt[2][0] >= 0 and lt[3][:4] == NO_MATCH and lt[3][5:] == (0, 0, -1)
    assert [i for i in range(14) if lmem[i][0] == -1] == sorted(free + [2, 3, 10, 11]) and all(lmem[i][2:5] == (0, 0, 0) for i in free + [2, 3, 10, 11])
    assert all(lmem[i][5] == -1 for i in free) and [lmem[i][5] for i in in_track] == [1, 1, 3, 4, 2, 2]
    assert (lsrc[free + [2, 3, 10, 11]] == 255).all() and len(lparts) == lmem[6][2] + lmem[7][2] > 0


def test_the_small_track_decode_case_is_the_constant_records(S, cases, host):
    d = cases["small"]["td"]
    rec, ch, mc = host("small", "one")["decode_tracks"]
    assert d["rows_of"] == [3, 33, 40, 0, 4] and d["tracks"] == [[], [1, 2], [3, 3], [0, 4, 0]] and d["packed"][3].tolist() == [0, 2, 6, 10]
    rec = TD.as_tuples(rec)
    assert rec[0] == rec[1] == TD.NOT_DECODED and rec[2] == (-1, -1, 0, 0, 0, 2, -1, -1) and rec[3][0] >= 0 and rec[3][5] == 3          # none, unusable, no seeds, ordinary
    assert (ch[:3] == 255).all() and (ch[3, :rec[3][2]] != 255).all()
    assert [i for i in range(15) if mc[i] == -1] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 14]
    # the decoder's INS / DEL are off: a string has one label a row, so among the usable words only the one without rows is no seed
    dec, _, _ = S.decode_words_host(*d["packed"][:3], cases["B"], DEFAULTS["dec_ins"], DEFAULTS["dec_dele"])
    assert dec["n_chars"].tolist() == [3, 0, 0, 0, 4] and dec["cost"][3] >= 0 and (dec["cost"][1:3] == -1).all()


def test_the_large_track_decode_case_sits_on_both_sides_of_the_resident_rows(cases, host):
    d = cases["large"]["td"]
    rows = [sum(d["rows_of"][w] for w in t) for t in d["tracks"]]
    assert RC.TD_RES_ROWS == 252 and rows[:3] == [288, 252, 253] and max(rows[3:]) < 64
    assert [d["rows_of"][w] for w in d["tracks"][0]] == [32] * 9 and all(0 < d["rows_of"][w] <= 32 for t in d["tracks"] for w in t)
    rec, ch, mc = host("large", "one")["decode_tracks"]
    assert (rec["cost"] >= 0).all() and (rec["n_used"] == d["packed"][4]).all() and (mc >= 0).all() and not (ch == 255).all(axis=1).any()
    assert (rec["n_edits"][:3] >= 1).all() and (rec["n_chars"][:3] == 32).all()          # the polish moves the strings of 32 labels


@pytest.mark.parametrize("name", ["one", "big"])
def test_the_large_case_has_no_empty_record(cases, host, name):
    h, r = host("large", name), cases["large"]["rows"]
    assert all(any(k > 0 for k in c) and sum(k + 1 for k in c) <= 32 for c in r["shapes"])          # a cut run in every word, every lattice usable
    assert r["tc"].sum() == len(r["mem"]) and (r["tc"] >= 1).all() and (r["tf"] == np.concatenate([[0], np.cumsum(r["tc"])[:-1]])).all()          # every slot in a track
    assert (h["match_words"][0]["entry"] >= 0).all() and (h["match_words"][0]["n_tried"] > 0).all()
    lm = h["lattice_match_words"][0]
    assert (lm["entry"] >= 0).all() and (lm["n_parts"] + lm["n_ins"] > 0).all() and (h["lattice_match_words"][1][:, 0] != 255).all()
    assert (h["split_words"][0]["n_parts"] >= r["n_of"]).all() and (r["n_of"] >= 1).all()
    assert (h["decode_words"][0]["cost"] >= 0).all() and (h["decode_words"][0]["n_chars"] >= 1).all()
    ld = h["lattice_decode_words"][0]
    assert (ld["cost"] >= 0).all() and (ld["n_parts"] >= 1).all()
    mt, mc = h["match_tracks"]
    assert (mt["entry"] >= 0).all() and (mt["n_used"] == r["tc"]).all() and (mc >= 0).all()
    lt, lmem, lsrc, _ = h["lattice_match_tracks"]
    assert (lt["entry"] >= 0).all() and (lt["n_used"] == r["tc"]).all() and (lmem["cost"] >= 0).all() and (lmem["word"] == r["mem"]).all()
    assert (lmem["n_parts"] + lmem["n_ins"] > 0).all() and (lsrc[:, 0] != 255).all()


def test_the_small_margin_track_and_line_cases_are_the_constant_records(cases, host):
    """Which records of the five newer stages' small case no input decides, and that the ordinary ones beside them are live."""
    h, c = host("small", "one"), cases["small"]
    check_small_margins(h)
    wg, lg = tuples(h["word_margins"][0]), tuples(h["lattice_margins"][0])
    assert all(m[0] >= 0 and 0 <= m[1] < n for m, n in zip(wg[2:], (9, 4, 3))) and all(m[0] >= 0 and m[7] > 0 for m in lg[3:])          # 9 runs: decoded by its rows, not by its lattice
    assert lg[3][4] >= 0 and lg[4][4] >= 0                     # ... and a cut margin in both ordinary words
    r = c["rows"]
    assert r["ltd_tracks"] == r["tracks"] + [[0, 0]] and r["ltd"][0].tolist() == [0, 2, 6, 10, 14] and len(r["ltd"][2]) == 18
    rec, ch, mem, src, parts = h["lattice_decode_tracks"]
    assert int(rec[2]["cost"]) >= 0 and int(rec[2]["n_used"]) == 2 and (ch[2, :int(rec[2]["n_chars"])] != 255).all() and (mem["cost"][[6, 7]] >= 0).all() and len(parts) > 0
    L = c["lines"]
    assert L["n_of"].tolist() == [0, RC.LINE_MAX + 1, 3] and L["first"].tolist() == [0, 0, RC.LINE_MAX + 1 + RC.GAP] and len(L["costs"]) == RC.LINE_MAX + 1 + 3 + 2 * RC.GAP
    assert L["no_line"].tolist() == [1025, 1026, 1030, 1031] and (L["gaps"][L["no_line"]] == (0, 255)).all()
    dec, lch, lsrc, wor = h["decode_lines"]
    assert int(dec[0]["cost"]) == int(cases["B"][65, 65]) and tuples(dec)[2][0] >= 0 and tuples(dec)[2][3] == 3 and (wor[1027:1030] >= 0).all() and lch[3 * 1027] != 255
    lm = tuples(h["line_margins"][0])
    assert lm[2][0] >= 0 and (h["line_margins"][1][1027:1030] >= 0).all() and (h["line_margins"][4][1028:1030] >= 0).all()


def test_the_large_margin_track_and_line_cases_have_no_empty_record(cases, host):
    h, c = host("large", "one"), cases["large"]
    wg, wrm, wrr, wra = h["word_margins"]
    n_of = c["rows"]["n_of"]
    assert (wg["margin"] >= 0).all() and all((wrm[w, :k] >= 0).all() and (wrr[w, :k] != 255).all() and (wra[w, :k] != 255).all() for w, k in enumerate(n_of))
    lg = h["lattice_margins"]
    ld = h["lattice_decode_words"][0]
    assert (lg[0]["read_margin"] >= 0).all() and (lg[0]["cut_margin"] >= 0).all() and (lg[0]["n_edges"] > 0).all()          # (a cut run in every word)
    assert all((lg[1][w, :k] >= 0).all() and (lg[3][w, :k] != 255).all() and (lg[4][w, :k] != 255).all() for w, k in enumerate(ld["n_parts"]))
    r = c["rows"]
    tf, tc, slots = r["ltd"]
    assert r["ltd_tracks"][:len(r["tracks"])] == r["tracks"] and len(tf) == len(r["tracks"]) + 32 and tc.sum() == len(slots) and (tc >= 1).all()          # every slot in a track
    rec, ch, mem, src, parts = h["lattice_decode_tracks"]
    assert (rec["cost"] >= 0).all() and (rec["n_used"] == tc).all() and (mem["cost"] >= 0).all() and (mem["word"] == slots).all() and (mem["n_parts"] + mem["n_ins"] > 0).all()
    assert (ch[:, 0] != 255).all() and (src[:, 0] != 255).all()
    L = c["lines"]
    assert len(L["no_line"]) == 0 and (L["n_of"] >= 1).all() and (L["n_of"][:17] == RC.LINE_MAX).all() and int(L["n_of"].sum()) == len(L["costs"])
    dec, lch, lsrc, wor = h["decode_lines"]
    assert (dec["cost"] >= 0).all() and (dec["n_sub"] == L["n_of"]).all() and (wor >= 0).all() and int(dec["n_breaks"].sum()) > 0          # (INS / DEL are off: a character a row)
    assert (lch.reshape(-1, 3)[:, 0][L["first"]] != 255).all() and (lsrc.reshape(-1, 3)[:, 0][L["first"]] != 0xFFFF).all()
    lm, rm, rr, ra, gm, gv = h["line_margins"]
    inner = np.setdiff1d(np.arange(len(rm)), L["first"])                 # (the first row of a line has no gap)
    assert (lm["margin"] >= 0).all() and (rm >= 0).all() and (rr != 255).all() and (ra != 255).all() and (gm[inner] >= 0).all() and (gv[inner] != 255).all()
    assert (lm["gap_margin"][L["n_of"] >= 2] >= 0).all()


def test_the_footprints(cases):
    small, large = cases["small"]["feet"], cases["large"]["feet"]
    tabs, splits, pieces, _ = RS.tables(small["items"])
    assert tabs[0][0][3] == 0 and small["items"][0][2].size == 0          # a footprint without a bit: no runs, no words
    assert [lw[3] for lw in tabs[0][1:]] == [2, 1, 1, 2] and [s[0] for s in splits] == [0, 1, 0, 0, 0, 2] and any(s != 0.0 for s in small["slopes"])
    ltabs, lsplits, lpieces, _ = RS.tables(large["items"])
    assert all(lw[3] >= 1 for lw in ltabs[0])                              # every footprint has runs
    cut = [any(s[0] > 0 for s in lsplits[lw[2]:lw[2] + lw[3]]) for lw in ltabs[0]]
    assert sum(cut[:64]) >= 60 and len(lpieces) >= 16 * len(pieces) and len(ltabs[1]) >= 16 * len(tabs[1])


# ---- 2. single-stage calls on one context --------------------------------------------------------------------------------------------------

def run_stage(f, name, c):
    """One entry point on a case: a tuple of arrays."""
    rows, lat, tr = _args(c)
    feet = (RC.W, RC.H, c["ft"], c["bits"])
    if name == "feet_words":
        return f.feet_words(*feet)
    if name == "feet_read":
        return f.feet_read(*feet, c["feet"]["slopes"])
    if name == "feet_split":
        got = f.feet_split(*feet, c["feet"]["slopes"])
        return tuple(got[k] for k in SPLIT_KEYS)
    if name == "match_words":
        return (f.match_words(*rows),)
    if name == "decode_words":
        return f.decode_words(*rows)
    if name == "decode_tracks":
        return f.decode_tracks(*c["td"]["packed"])
    if name == "word_margins":
        return f.word_margins(*rows)[:4]
    if name == "lattice_margins":
        return f.lattice_margins(*lat)[:6]
    if name == "lattice_decode_tracks":
        return f.lattice_decode_tracks(*lat, *c["rows"]["ltd"])
    if name in ("decode_lines", "line_margins"):
        return getattr(f, name)(*_lines(c))
    if name in ("match_tracks", "lattice_match_tracks"):
        return getattr(f, name)(*(rows if name == "match_tracks" else lat), *tr)
    return getattr(f, name)(*lat)


def run_round(f, c, reverse=False):
    return {name: run_stage(f, name, c) for name in (STAGES[::-1] if reverse else STAGES)}


def same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, i, np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:5].tolist() if a.shape == b.shape else (a.shape, b.shape))


def check_round(out, want, fresh, c, what):
    """A round against the host entry points (want), line_words_ref and the brand-new context's feet_read / feet_split (fresh)."""
    for name in STAGES[3:]:
        assert all(a is not None for a in want[name]), name
        same(out[name], want[name], (what, name))
    for table, a, b in zip(("line_words", "line_runs", "words"), LW.as_lists(*out["feet_words"]), LW.tables(c["feet"]["items"])):
        assert a == b, (what, "feet_words", table)
    for name in FEET_STAGES[1:]:
        same(out[name], fresh[name], (what, name))
    same(out["feet_read"][:3], out["feet_words"], (what, "the tables of feet_read"))


def fresh_feet(S, cascade_paths, load, c, split=(1, 4, 8)):
    """feet_read and feet_split of a case on a brand-new context, created and closed here."""
    g = S.ERFilter(params=S.Params(max_width=RC.W, max_height=RC.H, max_frames=1))
    try:
        g.load_cascade(0, cascade_paths[0]); g.load_cascade(1, cascade_paths[1])
        load(g)
        g.set_run_split(*split)
        return {name: run_stage(g, name, c) for name in FEET_STAGES[1:]}
    finally:
        g.close()


def check_small_constants(out):
    """The records of a small round that no input decides, slot by slot: a stale record of a larger call would stand in one of them."""
    mw = tuples(out["match_words"][0])
    assert mw[1][:4] == NO_MATCH and mw[1][5] == 0, "match_words: the word of 33 runs"
    lm, lsrc, _ = out["lattice_match_words"]
    for w in (1, 2):
        assert tuples(lm)[w][:4] == NO_MATCH and int(lm[w]["n_tried"]) == 0 and int(lm[w]["n_parts"]) == 0 and (lsrc[w] == 255).all(), ("lattice_match_words", w)
    assert int(lm[0]["n_parts"]) == 0 and tuples(out["split_words"][0])[0] == (0, 0, 0, 0)
    dw, ld = out["decode_words"][0], out["lattice_decode_words"][0]
    assert int(dw[1]["cost"]) == -1 and int(dw[1]["n_chars"]) == 0, "decode_words: the word of 33 runs"
    for w in (0, 1, 2):
        assert int(ld[w]["n_parts"]) == 0 and (w == 0 or int(ld[w]["cost"]) == -1), ("lattice_decode_words", w)
        assert w == 0 or (out["lattice_decode_words"][1][w] == 255).all(), ("lattice_decode_words", w)
    free, unusable = [0, 1, 4, 5, 8, 9, 12, 13], [2, 3]
    mt, mc = out["match_tracks"]
    assert tuples(mt)[0] == NO_MATCH + (0, 0, 0, -1) and tuples(mt)[1][:4] == NO_MATCH and tuples(mt)[1][5:] == (0, 0, -1)
    for i in free + unusable:
        assert int(mc[i]) == -1, ("match_tracks: member_cost", i)
    lt, lmem, lts, _ = out["lattice_match_tracks"]
    for g in (0, 1, 3):
        assert tuples(lt)[g][:4] == NO_MATCH and tuples(lt)[g][5:] == (0, 0, -1), ("lattice_match_tracks", g)
    for i in free + unusable + [10, 11]:
        assert int(lmem[i]["cost"]) == -1 and tuples(lmem)[i][2:5] == (0, 0, 0) and (lts[i] == 255).all(), ("lattice_match_tracks: member", i)
    for i in free:
        assert int(lmem[i]["word"]) == -1, ("lattice_match_tracks: member", i)
    rec, ch, tmc = out["decode_tracks"]
    assert TD.as_tuples(rec)[:3] == [TD.NOT_DECODED, TD.NOT_DECODED, (-1, -1, 0, 0, 0, 2, -1, -1)]
    assert (ch[:3] == 255).all(), "decode_tracks: the label bytes of an undecoded track"
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 14):
        assert int(tmc[i]) == -1, ("decode_tracks: member_cost", i)
    check_small_margins(out)


def check_small_margins(out):
    """... and those of the margins, the lattice track decode and the lines."""
    wg, wrm, wrr, wra = out["word_margins"]
    runs = [0, 33, 9, 4, 3]
    for w in (0, 1):
        assert tuples(wg)[w] == NO_MARGIN, ("word_margins", w)
    for w, n in enumerate(runs):          # the rows a word does not have, and every row of a word that is not decoded
        k = n if n <= 32 and w >= 2 else 0
        assert (wrm[w, k:] == -1).all() and (wrr[w, k:] == 255).all() and (wra[w, k:] == 255).all(), ("word_margins: rows", w)
    lg = out["lattice_margins"]
    for w in (0, 1, 2):
        assert tuples(lg[0])[w] == NO_LATTICE_MARGIN, ("lattice_margins", w)
        assert all((t[w] == -1).all() for t in lg[1:3]) and all((t[w] == 255).all() for t in lg[3:]), ("lattice_margins: parts", w)
    rec, ch, mem, src, parts = out["lattice_decode_tracks"]
    assert TD.as_tuples(rec)[:2] == [TD.NOT_DECODED] * 2 and TD.as_tuples(rec)[3:] == [TD.NOT_DECODED, (-1, -1, 0, 0, 0, 2, -1, -1)]          # none, unusable, (ordinary,) unusable, no seeds
    assert (ch[[0, 1, 3, 4]] == 255).all(), "lattice_decode_tracks: the label bytes of an undecoded track"
    in_track = {2: 1, 3: 1, 6: 3, 7: 4, 10: 2, 11: 2, 14: 0, 15: 0}
    for i in range(18):
        if i not in (6, 7):
            m = tuples(mem)[i]
            assert (m[0],) + m[2:5] == NO_MEMBER and m[5] == in_track.get(i, -1) and (src[i] == 255).all(), ("lattice_decode_tracks: member", i)
    assert len(parts) == int(mem[6]["n_parts"]) + int(mem[7]["n_parts"])
    dec, lch, lsrc, wor = out["decode_lines"]
    assert tuples(dec)[1] == NO_LINE and tuples(dec)[0][1:] == NO_LINE[1:], "decode_lines: the line of 1025 rows and the line without rows"
    nowhere = list(range(RC.LINE_MAX + 1 + RC.GAP)) + [len(wor) - 2, len(wor) - 1]          # the rows of the undecoded line and of no line
    assert (wor[nowhere] == -1).all() and (lch.reshape(-1, 3)[nowhere] == 255).all() and (lsrc.reshape(-1, 3)[nowhere] == 0xFFFF).all(), "decode_lines: rows"
    lm, rm, rr, ra, gm, gv = out["line_margins"]
    assert tuples(lm)[:2] == [NO_LINE_MARGIN] * 2, "line_margins: the line without rows and the line of 1025 rows"
    assert (rm[nowhere] == -1).all() and (gm[nowhere] == -1).all() and (rr[nowhere] == 255).all() and (ra[nowhere] == 255).all() and (gv[nowhere] == 255).all(), "line_margins: rows"


class Pools:
    """A pool of rows and a lattice pool on one context; every round adds its tracks to the slots 0 .. and reads every slot against the
    track match on the concatenation of everything the slots were given since the last reset, as test_track_pool.check does."""

    def __init__(self, S, f, cases, p=DEFAULTS):
        self.S, self.p = S, p
        small, large = cases["small"]["rows"], cases["large"]["rows"]
        self.cap = len(large["tf"]) + 1                        # (the last slot is never named)
        self.plain, self.lat = S.TrackPool(f, self.cap), S.TrackPool(f, self.cap, lattice=True)
        sp = np.concatenate([small["sp"], large["sp"]])
        sp["first_piece"][len(small["sp"]):] += len(small["pc"])
        first = np.concatenate([small["first"], large["first"] + len(small["rc"])]).astype(np.int32)
        self.both = (sp, np.concatenate([small["rc"], large["rc"]]), np.concatenate([small["pc"], large["pc"]]), first, np.concatenate([small["n_of"], large["n_of"]]))
        self.word0 = {"small": 0, "large": len(small["first"])}
        self.lists = [[] for _ in range(self.cap)]

    def close(self):
        self.plain.close(); self.lat.close()

    def bytes(self):
        return self.plain.info()["device_bytes"], self.lat.info()["device_bytes"]

    def reset(self):
        """After a change of the lexicon: both pools are stale, as their contract says, until they are reset."""
        for p in (self.plain, self.lat):
            assert p.info()["stale"]
            with pytest.raises(self.S.StrErError) as e:
                p.read([0])
            assert e.value.code == -6
            p.reset()
            assert not p.info()["stale"] and p.info()["in_use"] == 0
        self.lists = [[] for _ in range(self.cap)]

    def round(self, size, c, words, what):
        r = c["rows"]
        rows, lat, tr = _args(c)
        slots = np.arange(len(r["tf"]), dtype=np.int32)
        self.plain.add(*rows, *tr, slots)
        self.lat.add_lattice(*lat, *tr, slots)
        for g, t in enumerate(r["tracks"]):
            self.lists[g] += [w + self.word0[size] for w in t]
        every = np.arange(self.cap, dtype=np.int32)
        setting = (self.p["fold"], self.p["ins"], self.p["dele"], self.p["band"], self.p["split"])
        for pool, rows_of in ((self.plain, (self.both[1], self.both[3], self.both[4])), (self.lat, self.both)):
            got, want = pool.read(every), pool_reference(self.S, rows_of, self.lists, words, setting)
            assert got.dtype == self.S.POOL_MATCH_DTYPE and got.tolist() == want.tolist(), (what, [(s, tuple(a), tuple(b)) for s, a, b in zip(every, got, want) if a != b][:5])
            assert tuple(got[self.cap - 1]) == POOL_EMPTY and pool.info()["in_use"] == sum(1 for t in self.lists if t)
        if not self.lists[0]:
            assert tuple(self.plain.read([0])[0]) == POOL_EMPTY == tuple(self.lat.read([0])[0]), (what, "a slot that was only given a track of none")


def stats(f, pools):
    return {"run_atlas_stats": f.run_atlas_stats(), "run_split_stats": f.run_split_stats(), "lattice_decode_stats": (f.lattice_decode_stats(),),
            "lattice_match_stats": (f.lattice_match_stats(),), "lattice_track_stats": (f.lattice_track_stats(),), "pool device_bytes": pools.bytes(),
            "lattice_track_decode_stats": (f.lattice_track_decode_stats(),), "line_decode_stats": (f.line_decode_stats()["table_bytes"],),
            "line_margin_stats": (f.line_margin_stats()["table_bytes"],)}


@pytest.mark.gpu
def test_single_stage_rounds_on_one_context(S, cascade_paths, tmp_path_factory, oracle, cases, host):
    path, _ = _shipped(S, tmp_path_factory, 5)
    load = lambda g: g.load_svm_model(path, 1800)
    fresh = {size: fresh_feet(S, cascade_paths, load, cases[size]) for size in RC.SIZES}
    f = S.ERFilter(params=S.Params(max_width=RC.W, max_height=RC.H, max_frames=1))
    pools = None
    try:
        f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
        load(f)
        f.set_lexicon(cases["lex"]["one"])
        f.set_bigram(cases["B"])
        ws = f.workspace_bytes()
        pools = Pools(S, f, cases)
        first_small, seen = {}, {}

        def go(n, size, name, reverse=False):
            what = f"round {n}: {size} under the lexicon '{name}'" + (", in reverse order" if reverse else "")
            before = stats(f, pools)
            out = run_round(f, cases[size], reverse)
            check_round(out, host(size, name), fresh[size], cases[size], what)
            pools.round(size, cases[size], cases["lex"][name], what)
            if size == "small":
                check_small_constants(out)
                if name in first_small:                        # every small round under a lexicon equals the first under it, byte for byte
                    for stage in STAGES:
                        same(out[stage], first_small[name][stage], (what, stage, "against the first small round"))
                    assert stats(f, pools) == before, what     # ... and no buffer grows for it
                first_small.setdefault(name, out)
                for stage in STAGES[:4] + STAGES[5:7] + STAGES[10:]:          # what the lexicon does not enter equals round 1 under any
                    same(out[stage], first_small["one"][stage], (what, stage, "against round 1"))
            seen[n] = stats(f, pools)
            assert f.workspace_bytes() == ws, what
            return out

        out = go(1, "small", "one")
        # feet_read and feet_split once against their modules' references
        feet = cases["small"]["feet"]
        tabs, q, _ = RR.features(oracle, feet["items"], feet["slopes"])
        assert list(LW.as_lists(*out["feet_read"][:3])) == list(tabs) and out["feet_read"][4].shape == q.shape and (out["feet_read"][4] == q).all()
        stabs, splits, pieces, line_of = RS.tables(feet["items"])
        pq, _ = RS.piece_features(oracle, feet["items"], pieces, line_of, feet["slopes"])
        got = dict(zip(SPLIT_KEYS, out["feet_split"]))
        assert list(RS.as_lists(got["splits"], got["pieces"])) == [splits, pieces] and list(LW.as_lists(*out["feet_split"][:3])) == list(stabs)
        assert got["piece_q"].shape == pq.shape and (got["piece_q"] == pq).all() and len(got["piece_reads"]) == len(pieces)
        go(2, "large", "one")
        for k in seen[1]:                                      # the buffers grow between the rounds 1 and 2
            assert all(b > a for a, b in zip(seen[1][k], seen[2][k])), (k, seen[1][k], seen[2][k])
        go(3, "small", "one")
        go(4, "large", "one", reverse=True)
        assert seen[4] == seen[2]
        go(5, "small", "one", reverse=True)
        f.set_lexicon(cases["lex"]["big"])
        pools.reset()
        go(6, "small", "big")
        go(6, "large", "big")
        f.set_lexicon(cases["lex"]["one"])
        pools.reset()
        go(7, "small", "one")
        assert f.workspace_bytes() == ws
    finally:
        if pools:
            pools.close()
        f.close()


# ---- 3. the fused call and the handover ----------------------------------------------------------------------------------------------------

def tables_of(res):
    return {k: getattr(res, k) for k in FUSED_TABLES}


def same_tables(a, b, what):
    for k in FUSED_TABLES:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.gpu
def test_the_fused_call_and_the_single_stage_calls_take_turns(S, cascade_paths, cases, lex, proto):  # noqa: F811
    _, _, prm, model, uniform, _, words = lex
    table = proto[8]
    p = dict(DEFAULTS, ins=INS, dele=DEL, band=BAND, num=NUM, den=DEN, split=SPLIT, dec_ins=DEC_INS, dec_dele=DEC_DEL)
    load = lambda g: g.load_svm_model(model, 1800)

    def context():
        g = S.ERFilter(params=S.Params(max_width=640, max_height=480, max_frames=2, n_pyr_levels=prm.n_pyr_levels))
        g.load_cascade(0, cascade_paths[0]); g.load_cascade(1, cascade_paths[1])
        load(g)
        g.set_run_split(NUM, DEN, SPLIT)
        g.set_bigram(table)
        g.set_word_decode(DEC_INS, DEC_DEL)
        g.set_lexicon(words, fold_case=True)
        g.set_word_match(INS, DEL, BAND)
        g.set_word_margin(True); g.set_lattice_margin(True); g.set_lattice_track_decode(True); g.set_line_decode(True); g.set_line_margin(True)
        return g

    busy = np.stack([uniform[0], uniform[0]])                  # the S-text frame of seed 2, twice: the word tracks have two members
    ragged = [S.synth.stext_bgr(S.synth.frame_seed(971), 333, 211)]
    g = context()
    try:
        alone = tables_of(g.text_detect_list(ragged, GROUPED, **FUSED))
    finally:
        g.close()
    fresh = {size: fresh_feet(S, cascade_paths, load, cases[size], (NUM, DEN, SPLIT)) for size in RC.SIZES}
    f = context()
    try:
        one = tables_of(f.text_detect(busy, GROUPED, **FUSED))
        assert len(one["word_tracks"]) > 0 and int(one["word_tracks"]["count"].max()) >= 2 and (one["run_splits"]["n_cuts"] > 0).any()          # the scene's conditions
        assert (one["lattice_track_members"]["n_parts"] > 0).any() and (one["track_decodes"]["cost"] >= 0).any() and len(one["split_parts"]) > len(one["line_runs"])
        assert (one["word_margins"]["margin"] >= 0).any() and (one["lattice_margins"]["cut_margin"] >= 0).any() and (one["lattice_track_decodes"]["cost"] >= 0).any()
        assert (one["line_decodes"]["n_breaks"] > 0).any() and (one["line_margins"]["margin"] >= 0).any() and len(one["line_decode_word_of_row"]) == len(one["split_parts"])
        blank = tables_of(f.text_detect(np.full((480, 640, 3), 128, np.uint8), GROUPED, **FUSED))
        for k in READING_TABLES:
            assert len(blank[k]) == 0, k
        same_tables(tables_of(f.text_detect_list(ragged, GROUPED, **FUSED)), alone, "the list call against a brand-new context")
        ws = f.workspace_bytes()          # (the detector's node records and content-sized tables are accounted and grow with the first call of each kind; the reading chain's are not)
        same_tables(tables_of(f.text_detect(busy, GROUPED, **FUSED)), one, "call 4 against call 1")
        for size in RC.SIZES:
            want = host_round(S, cases[size], words, table, p)
            check_round(run_round(f, cases[size]), want, fresh[size], cases[size], f"{size} between the fused calls")
            assert f.workspace_bytes() == ws
        same_tables(tables_of(f.text_detect(busy, GROUPED, **FUSED)), one, "call 6 against call 1")
        assert f.workspace_bytes() == ws
    finally:
        f.close()
