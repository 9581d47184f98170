"""STR_ER_WANT_LATTICE_TRACK in the detect calls, on the scene and the prototype model of test_lattice_match_pipeline.py (a model made from
the call's own pieces, with which most words have a cut run), every frame submitted twice so that the word tracks have several members: the
flag's four tables are exactly what str_er_lattice_match_tracks gives on the same result's run_splits, run_costs, piece_costs, words and
word tracks, and what the numpy reference gives (lattice_track_ref.py); some member takes more parts than it has runs; every other
table byte for byte that of the call without the flag; the flag's rules."""
import numpy as np
import pytest

import lattice_track_ref as LT
import word_match_ref as WM
from test_frame_lines import GROUPED
from test_lattice_decode_pipeline import proto  # noqa: F401  (the fixture)
from test_lattice_match_pipeline import BOTH, BAND, DEL, INS, MATCH_TABLES, OTHER_TABLES, lex  # noqa: F401  (the fixture)
from test_run_split_pipeline import SPLIT, scene  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
TRACK_TABLES = ("lattice_track_matches", "lattice_track_members", "lattice_track_src", "lattice_track_parts")
READ_TABLES = ("word_links", "word_tracks", "word_track_members", "word_track_of_words", "track_matches", "track_member_costs", "line_links", "line_tracks",
               "text_tracks", "text_track_members")
TRACKED = dict(want_line_links=True, want_track_read=True, want_lattice_match=True, **BOTH)


@pytest.fixture(scope="module")
def calls(lex):  # noqa: F811
    """The scene's two frames, each twice, detected without and with the flag."""
    S, g, prm, model, uniform, crops, words = lex
    frames = np.stack([uniform[0], uniform[0], uniform[1], uniform[1]])
    before = g.lattice_track_stats()
    base = g.text_detect(frames, GROUPED, **TRACKED)
    assert g.lattice_track_stats() == before == 0                        # (a call without the flag makes none of the flag's buffers)
    res = g.text_detect(frames, GROUPED, want_lattice_track=True, **TRACKED)
    return S, g, frames, words, base, res


def _cut_members(res):
    first, n_of, cuts = res.words["first_run"], res.words["n_runs"], res.run_splits["n_cuts"]
    return [bool((cuts[first[w]:first[w] + n_of[w]] > 0).any()) for w in res.word_track_members]


def test_the_model_leaves_members_with_a_cut_in_tracks_of_several(calls):
    """The guard of this file: without a member with a cut run, and without a track of several members, the tests below would show
    nothing.  It fails, and does not skip."""
    S, g, frames, words, base, res = calls
    assert len(res.word_tracks) > 0 and int(res.word_tracks["count"].max()) >= 2
    assert sum(_cut_members(res)) >= 1
    many = res.word_tracks[res.word_tracks["count"] >= 2]
    assert any(any(_cut_members(res)[int(t["first"]):int(t["first"]) + int(t["count"])]) for t in many)


def test_detect_equals_the_entry_point_and_the_reference_on_the_calls_own_tables(calls):
    S, g, frames, words, base, res = calls
    first, n_of = res.words["first_run"], res.words["n_runs"]
    tf, tc, mem = res.word_tracks["first"], res.word_tracks["count"], res.word_track_members
    rec, mrec, src, parts = res.lattice_track_matches, res.lattice_track_members, res.lattice_track_src, res.lattice_track_parts
    assert rec.dtype == S.TRACK_MATCH_DTYPE and len(rec) == len(tf) and mrec.dtype == S.LATTICE_TRACK_MEMBER_DTYPE and len(mrec) == len(mem) and src.shape == (len(mem), 32)
    got = g.lattice_match_tracks(res.run_splits, res.run_costs, res.piece_costs, first, n_of, tf, tc, mem)
    for a, b in zip((rec, mrec, src, parts), got):
        assert a.tobytes() == b.tobytes()
    host = S.lattice_match_tracks_host(res.run_splits, res.run_costs, res.piece_costs, first, n_of, tf, tc, mem, words, True, INS, DEL, BAND, SPLIT)
    for a, b in zip((rec, mrec, src, parts), host):
        assert a.tobytes() == b.tobytes()
    want = LT.match_tracks(res.run_splits, res.run_costs, res.piece_costs, first, n_of, tf, tc, mem, WM.Lexicon(words, True), INS, DEL, BAND, SPLIT)
    assert LT.as_tuples(rec) == want[0] and LT.members_as_tuples(mrec) == want[1] and (src == want[2]).all()
    assert np.stack([parts["run"], parts["piece"]], 1).tolist() == want[3].tolist()
    # some member takes more parts than it has runs, and the texts follow the records
    assert (mrec["word"] == mem).all() and (mrec["n_parts"] > n_of[mem]).any()
    print(f"{len(tf)} word tracks, {len(mem)} members, {int((rec['entry'] >= 0).sum())} matched, {int((mrec['n_parts'] > n_of[mem]).sum())} members with more parts than runs, "
          f"{int((rec['entry'] != res.track_matches['entry']).sum())} tracks with another entry than the track match's")
    for k in range(len(tf)):
        e = int(rec[k]["entry"])
        assert res.word_track_lattice_text(k) == (words[e] if e >= 0 else res.word_text(int(res.word_tracks[k]["rep"])))
    for i in range(len(mem)):
        own = res.track_member_lattice_parts(i)
        assert len(own) == int(mrec[i]["n_parts"]) and ((own["run"] >= first[mem[i]]) & (own["run"] < first[mem[i]] + n_of[mem[i]])).all()
    of = res.word_track_of_words
    for k, t in enumerate(res.text_tracks):
        lw = res.line_words[int(t["rep"])]
        ws = range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))
        assert res.text_track_lattice_match_text(k) == " ".join(res.word_track_lattice_text(int(of[w])) if of[w] >= 0 else res.word_text(w) for w in ws)
    # where every member of a track is uncut the record is the track match's on the unsplit runs
    plain, mc = g.match_tracks(res.run_costs, first, n_of, tf, tc, mem)
    cut = _cut_members(res)
    for k in range(len(tf)):
        a, n = int(tf[k]), int(tc[k])
        if not any(cut[a:a + n]):
            assert rec[k].tobytes() == plain[k].tobytes() and mrec["cost"][a:a + n].tolist() == mc[a:a + n].tolist()
        elif int(plain[k]["n_tried"]) > 0 and int(rec[k]["n_used"]) == n:
            assert int(rec[k]["n_tried"]) >= int(plain[k]["n_tried"]) and 0 <= int(rec[k]["cost"]) <= int(plain[k]["cost"])


def test_every_other_table_is_that_of_the_call_without_the_flag(calls):
    S, g, frames, words, base, res = calls
    for k in OTHER_TABLES + MATCH_TABLES + READ_TABLES:
        assert getattr(base, k).tobytes() == getattr(res, k).tobytes(), k
    for k in TRACK_TABLES:
        with pytest.raises(ValueError):
            getattr(base, k)
    again = g.text_detect(frames, GROUPED, want_lattice_track=True, **TRACKED)
    for k in TRACK_TABLES:
        assert getattr(again, k).tobytes() == getattr(res, k).tobytes(), k
    assert g.lattice_track_stats() > 0


def test_the_refusals_name_the_flag(calls):
    S, g, frames, words, base, res = calls
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS
    want = (flags | S.WANT_RUN_READ | S.WANT_RUN_SPLIT | S.WANT_WORD_MATCH | S.WANT_LINE_LINKS | S.WANT_TRACK_READ | S.WANT_LATTICE_MATCH | S.WANT_LATTICE_TRACK)
    for name in ("WANT_TRACK_READ", "WANT_LATTICE_MATCH", "WANT_RUN_SPLIT", "WANT_WORD_MATCH", "WANT_LINE_LINKS", "WANT_RUN_READ"):
        with pytest.raises(S.StrErError) as e:
            g.text_detect(frames, want & ~getattr(S, name))
        assert e.value.code == -1 and "STR_ER_WANT_LATTICE_TRACK needs" in str(e.value) and "STR_ER_" + name in str(e.value), name
    planes = g.compute_channels(frames[0])
    with pytest.raises(S.StrErError) as e:                               # the per-plane calls
        g.detect_planes(planes[:1], S.STAGE_ALL | (want & ~GROUPED))
    assert e.value.code == -1 and "STR_ER_WANT_LATTICE_TRACK" in str(e.value)
    with pytest.raises(S.StrErError) as e:                               # the strip path (the flags are judged before the blobs are read)
        g.strip_merge(frames[0], [b"none"], stages=want)
    assert e.value.code == -1 and "STR_ER_WANT_LATTICE_TRACK" in str(e.value) and "strip" in str(e.value)
    g.set_lexicon([])
    try:
        with pytest.raises(S.StrErError) as e:                           # no lexicon: the matcher's rule
            g.text_detect(frames, want)
        assert e.value.code == -6 and "lexicon" in str(e.value)
    finally:
        g.set_lexicon(words)
    good = g.text_detect(frames, GROUPED, want_lattice_track=True, **TRACKED)      # (the context is usable afterwards)
    for k in TRACK_TABLES + MATCH_TABLES:
        assert getattr(good, k).tobytes() == getattr(res, k).tobytes(), k
    # a grouped call without lines: empty tables, not an error
    blank = g.text_detect(np.full((120, 160, 3), 128, np.uint8), want)
    assert len(blank.texts) == 0 and len(blank.lattice_track_matches) == len(blank.lattice_track_members) == len(blank.lattice_track_parts) == 0
    assert blank.lattice_track_src.shape == (0, 32)
