"""STR_ER_WANT_TRACK_DECODE in the detect calls, on the 16-frame video of test_track_read_pipeline.py with the shipped model and no
lexicon set: the call succeeds, its records equal decode_tracks on the call's own rows, words and tracks (with want_run_split the rows
of the words' parts, rebuilt as the decoder's pipeline test does), every other table is byte for byte that of the call without the
flag, the links and tracks equal those of a STR_ER_WANT_TRACK_READ call, and the flag's refusals leave the context usable."""
import numpy as np
import pytest

import track_decode_ref as TD
from test_frame_lines import GROUPED
from test_line_links import make_video
from test_svm_exact import _shipped

pytestmark = pytest.mark.gpu
TABLES = ("line_words", "line_runs", "words", "run_reads", "run_features", "line_feet", "line_pairs", "frame_lines", "frame_line_members", "masks", "mask_bits",
          "line_links", "line_tracks", "text_tracks", "text_track_members", "word_decodes", "word_decode_chars", "word_decode_src", "run_costs", "run_probs")
LINKS = ("word_links", "word_tracks", "word_track_members", "word_track_of_words")
NEW = ("track_decodes", "track_decode_chars", "track_decode_member_costs")
WANTS = dict(want_masks=True, want_frame_lines=True, want_line_links=True, want_line_words=True, want_run_read=True, want_word_decode=True)


@pytest.fixture(scope="module")
def scene(S, cascade_paths, tmp_path_factory):
    path, m = _shipped(S, tmp_path_factory, 5)
    prm = S.Params(max_width=640, max_height=480, max_frames=16, n_pyr_levels=3)
    f = S.ERFilter(params=prm)
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    f.load_svm_model(path, 1800)
    frames, seg_of = make_video(S)
    first = f.text_detect_list(frames, GROUPED, want_frame_lines=True, want_line_words=True, want_run_read=True)
    read = [t for t in sorted({first.word_text(w) for w in range(len(first.words))}) if 1 <= len(t) <= 32]
    table = S.bigram_from_words(read)
    f.set_bigram(table)
    plain = f.text_detect_list(frames, GROUPED, **WANTS)
    res = f.text_detect_list(frames, GROUPED, want_track_decode=True, **WANTS)          # no lexicon is set
    yield S, f, frames, read, table, plain, res
    f.close()


def check_entry_point(f, res, rows=None):
    """The call's records against decode_tracks on its own rows (rows: (costs, first, n) where they are not the runs'), words and tracks."""
    costs, first, n_of = rows if rows is not None else (res.run_costs, res.words["first_run"], res.words["n_runs"])
    td, ch, mc = f.decode_tracks(costs, first, n_of, res.word_tracks["first"], res.word_tracks["count"], res.word_track_members)
    assert td.tobytes() == res.track_decodes.tobytes() and ch.tobytes() == res.track_decode_chars.tobytes()
    assert mc.tobytes() == res.track_decode_member_costs.tobytes()
    return costs, first, n_of


def test_list_call_without_a_lexicon(scene):
    S, f, frames, read, table, plain, res = scene
    assert len(res.word_tracks) > 0 and res.word_tracks["count"].max() >= 4
    assert len(res.track_decodes) == len(res.word_tracks) and res.track_decode_chars.shape == (len(res.word_tracks), 32)
    assert len(res.track_decode_member_costs) == len(res.word_track_members)
    costs, first, n_of = check_entry_point(f, res)
    # ... and the reference on a few tracks, the longest among them
    order = np.argsort(-res.word_tracks["count"], kind="stable")[:3].tolist() + [len(res.word_tracks) - 1]
    for g in order:
        t = res.word_tracks[g]
        members = [int(w) for w in res.word_track_members[int(t["first"]):int(t["first"]) + int(t["count"])]]
        rec, s, own, _ = TD.decode_track(costs, first, n_of, members, table)
        assert TD.as_tuples(res.track_decodes[g:g + 1]) == [rec] and list(res.track_decode_chars[g, :len(s)]) == s
        assert res.track_decode_member_costs[int(t["first"]):int(t["first"]) + int(t["count"])].tolist() == own
    # every other table is that of the call without the flag
    for k in NEW + LINKS:
        with pytest.raises(ValueError):
            getattr(plain, k)
    for k in TABLES:
        assert getattr(plain, k).tobytes() == getattr(res, k).tobytes(), k
    with pytest.raises(ValueError):
        res.track_matches
    # the texts
    track_of = res.word_track_of_words
    for g, d in enumerate(res.track_decodes):
        want = "".join(S.ocr_char(int(a)) for a in res.track_decode_chars[g, :int(d["n_chars"])]) if int(d["cost"]) >= 0 else res.word_text(int(res.word_tracks[g]["rep"]))
        assert res.word_track_decode_text(g) == want
    for k, t in enumerate(res.text_tracks):
        lw = res.line_words[int(t["rep"])]
        ws = range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))
        assert res.text_track_decode_text(k) == " ".join(res.word_track_decode_text(int(track_of[w])) if track_of[w] >= 0 else res.word_text(w) for w in ws)
    d = res.track_decodes
    print("word tracks", len(d), "decoded", int((d["cost"] >= 0).sum()), "edits", np.bincount(d["n_edits"]).tolist(), "converged", int(d["converged"].sum()))


def test_beside_the_run_split_and_other_parameters(scene):
    S, f, frames, read, table, plain, res = scene
    split = f.text_detect_list(frames, GROUPED, want_run_split=True, want_track_decode=True, **WANTS)
    rows = np.array([split.run_costs[int(p["run"])] if int(p["piece"]) < 0 else split.piece_costs[int(p["piece"])] for p in split.split_parts],
                    np.uint8).reshape(-1, 65)
    check_entry_point(f, split, (rows, split.word_splits["first_part"], split.word_splits["n_parts"]))
    for k in LINKS:                                           # the links and the tracks are those of the words: the split moves none
        assert getattr(split, k).tobytes() == getattr(res, k).tobytes(), k
    alone = f.text_detect_list(frames, GROUPED, want_run_split=True, **WANTS)
    for k in TABLES + ("run_splits", "run_pieces", "piece_reads", "piece_costs", "split_parts", "word_splits"):
        assert getattr(alone, k).tobytes() == getattr(split, k).tobytes(), k
    f.set_track_decode(40, 90, 1)
    f.set_word_decode(64, 64)
    try:
        other = f.text_detect_list(frames, GROUPED, want_track_decode=True, **WANTS)
        check_entry_point(f, other)
        assert other.track_decodes["n_edits"].max() <= 1
    finally:
        f.set_track_decode()
        f.set_word_decode()


def test_links_and_tracks_equal_those_of_a_track_read_call(scene):
    S, f, frames, read, table, plain, res = scene
    f.set_lexicon(read)
    try:
        tr = f.text_detect_list(frames, GROUPED, want_word_match=True, want_track_read=True, **WANTS)
        both = f.text_detect_list(frames, GROUPED, want_word_match=True, want_track_read=True, want_track_decode=True, **WANTS)
        match = f.text_detect_list(frames, GROUPED, want_word_match=True, want_track_decode=True, **WANTS)
    finally:
        f.set_lexicon([])
    for k in LINKS:
        assert getattr(tr, k).tobytes() == getattr(res, k).tobytes() == getattr(both, k).tobytes() == getattr(match, k).tobytes(), k
    for k in ("track_matches", "track_member_costs", "word_matches"):
        assert getattr(tr, k).tobytes() == getattr(both, k).tobytes(), k
    with pytest.raises(ValueError):
        match.track_matches                                   # the matcher beside the track decode: no track match without its flag
    for k in NEW + ("word_decodes", "word_decode_chars"):     # the decoder's rows stay unfolded beside a folding matcher
        assert getattr(both, k).tobytes() == getattr(res, k).tobytes() == getattr(match, k).tobytes(), k
    with pytest.raises(ValueError):
        tr.track_decodes


def test_flag_rules_leave_the_context_usable(scene):
    S, f, frames, read, table, plain, res = scene
    two = np.stack(frames[:2])
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS | S.WANT_RUN_READ
    with pytest.raises(S.StrErError) as e:                    # without STR_ER_WANT_LINE_LINKS
        f.text_detect(two, flags | S.WANT_WORD_DECODE | S.WANT_TRACK_DECODE)
    assert e.value.code == -1 and "STR_ER_WANT_TRACK_DECODE" in str(e.value)
    with pytest.raises(S.StrErError) as e:                    # without STR_ER_WANT_WORD_DECODE
        f.text_detect(two, flags | S.WANT_LINE_LINKS | S.WANT_TRACK_DECODE)
    assert e.value.code == -1 and "STR_ER_WANT_TRACK_DECODE" in str(e.value)
    planes = f.compute_channels(frames[0])
    with pytest.raises(S.StrErError) as e:                    # the per-plane calls
        f.detect_planes(planes[:1], S.STAGE_ALL | S.WANT_FRAME_LINES | S.WANT_LINE_LINKS | S.WANT_LINE_WORDS | S.WANT_RUN_READ | S.WANT_WORD_DECODE | S.WANT_TRACK_DECODE)
    assert e.value.code == -1 and "STR_ER_WANT_TRACK_DECODE" in str(e.value)
    f.set_bigram(None)
    try:
        with pytest.raises(S.StrErError) as e:                # without a table
            f.text_detect(two, flags | S.WANT_LINE_LINKS | S.WANT_WORD_DECODE | S.WANT_TRACK_DECODE)
        assert e.value.code == -6 and "bigram" in str(e.value)
    finally:
        f.set_bigram(table)
    # a grouped call without lines: empty tables, not an error
    blank = f.text_detect(np.full((120, 160, 3), 128, np.uint8), flags | S.WANT_LINE_LINKS | S.WANT_WORD_DECODE | S.WANT_TRACK_DECODE)
    assert len(blank.texts) == 0 and all(len(getattr(blank, k)) == 0 for k in NEW + LINKS)
    good = f.text_detect_list(frames, GROUPED, want_track_decode=True, **WANTS)
    for k in NEW + LINKS:
        assert getattr(good, k).tobytes() == getattr(res, k).tobytes(), k
