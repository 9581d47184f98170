"""str_er_set_lattice_track_decode in the detect calls, on the 16-frame video of test_track_decode_pipeline.py with the shipped model and
no lexicon set: with the setting on and both STR_ER_WANT_TRACK_DECODE and STR_ER_WANT_LATTICE_DECODE the result's new tables equal
lattice_decode_tracks on the result's own splits, rows and tracks; with the setting off every table of the same call is byte for byte
that of a context that never heard of the setting; with either flag missing the new tables are absent and nothing else moves; a
FrameStream's contexts honour the setting; and the call runs on a reused context that grows and shrinks between calls."""
import numpy as np
import pytest

import lattice_track_decode_ref as R
from test_frame_lines import GROUPED
from test_line_links import make_video
from test_svm_exact import _shipped

pytestmark = pytest.mark.gpu
TABLES = ("line_words", "line_runs", "words", "run_reads", "run_features", "line_feet", "line_pairs", "frame_lines", "frame_line_members", "masks", "mask_bits",
          "line_links", "line_tracks", "text_tracks", "text_track_members", "word_decodes", "word_decode_chars", "word_decode_src", "run_costs", "run_probs",
          "run_splits", "run_pieces", "piece_reads", "piece_costs", "split_parts", "word_splits")
LINKS = ("word_links", "word_tracks", "word_track_members", "word_track_of_words")
TRACK = ("track_decodes", "track_decode_chars", "track_decode_member_costs")
LATTICE = ("lattice_decodes", "lattice_decode_chars", "lattice_decode_src", "lattice_parts")
NEW = ("lattice_track_decodes", "lattice_track_decode_chars", "lattice_track_decode_members", "lattice_track_decode_src", "lattice_track_decode_parts")
WANTS = dict(want_masks=True, want_frame_lines=True, want_line_links=True, want_line_words=True, want_run_read=True, want_word_decode=True, want_run_split=True)
BOTH = dict(want_track_decode=True, want_lattice_decode=True)


def new_filter(S, cascade_paths, path, table, frames=16):
    f = S.ERFilter(params=S.Params(max_width=640, max_height=480, max_frames=frames, n_pyr_levels=3))
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    f.load_svm_model(path, 1800)
    if table is not None:
        f.set_bigram(table)
    return f


@pytest.fixture(scope="module")
def scene(S, cascade_paths, tmp_path_factory):
    path, m = _shipped(S, tmp_path_factory, 5)
    frames, seg_of = make_video(S)
    f = new_filter(S, cascade_paths, path, None)
    first = f.text_detect_list(frames, GROUPED, want_frame_lines=True, want_line_words=True, want_run_read=True)
    read = [t for t in sorted({first.word_text(w) for w in range(len(first.words))}) if 1 <= len(t) <= 32]
    table = S.bigram_from_words(read)
    f.set_bigram(table)
    fresh = new_filter(S, cascade_paths, path, table)          # a context that never hears of the setting
    plain = fresh.text_detect_list(frames, GROUPED, **BOTH, **WANTS)
    fresh.close()
    f.set_lattice_track_decode(True)
    res = f.text_detect_list(frames, GROUPED, **BOTH, **WANTS)
    yield S, f, frames, table, plain, res, path, cascade_paths
    f.close()


def check_entry_point(f, res):
    """The call's new tables against lattice_decode_tracks on its own splits, rows, words and tracks."""
    got = f.lattice_decode_tracks(res.run_splits, res.run_costs, res.piece_costs, res.words["first_run"], res.words["n_runs"], res.word_tracks["first"],
                                  res.word_tracks["count"], res.word_track_members)
    for k, a in zip(NEW, got):
        assert a.tobytes() == getattr(res, k).tobytes(), k


def test_the_setting_with_both_flags(scene):
    S, f, frames, table, plain, res, _, _ = scene
    assert len(res.word_tracks) > 0 and res.word_tracks["count"].max() >= 4
    assert len(res.lattice_track_decodes) == len(res.word_tracks) and res.lattice_track_decode_chars.shape == (len(res.word_tracks), 32)
    assert len(res.lattice_track_decode_members) == len(res.word_track_members) and res.lattice_track_decode_src.shape == (len(res.word_track_members), 32)
    check_entry_point(f, res)
    host = S.lattice_decode_tracks_host(res.run_splits, res.run_costs, res.piece_costs, res.words["first_run"], res.words["n_runs"], res.word_tracks["first"],
                                        res.word_tracks["count"], res.word_track_members, table)
    for k, a in zip(NEW, host):
        assert a.tobytes() == getattr(res, k).tobytes(), k
    # the identities on the call's own tables
    d, m = res.lattice_track_decodes, res.lattice_track_decode_members
    for g, t in enumerate(res.word_tracks):
        own = m[int(t["first"]):int(t["first"]) + int(t["count"])]
        if int(d[g]["cost"]) >= 0:
            assert int(d[g]["cost"]) == int(d[g]["lm_cost"]) + int(own["cost"][own["cost"] >= 0].sum()) and int(d[g]["cost"]) <= int(d[g]["seed_cost"])
            assert all(int(o["n_parts"]) - int(o["n_del"]) + int(o["n_ins"]) == int(d[g]["n_chars"]) for o in own if int(o["cost"]) >= 0)
    assert (m["word"] == res.word_track_members).all()
    assert len(res.lattice_track_decode_parts) == int(m["n_parts"].sum())
    # the texts and the parts of a slot
    for g, r in enumerate(d):
        want = "".join(S.ocr_char(int(a)) for a in res.lattice_track_decode_chars[g, :int(r["n_chars"])]) if int(r["cost"]) >= 0 else res.word_text(int(res.word_tracks[g]["rep"]))
        assert res.word_track_lattice_decode_text(g) == want
    track_of = res.word_track_of_words
    for k, t in enumerate(res.text_tracks):
        lw = res.line_words[int(t["rep"])]
        ws = range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))
        assert res.text_track_lattice_decode_text(k) == " ".join(res.word_track_lattice_decode_text(int(track_of[w])) if track_of[w] >= 0 else res.word_text(w) for w in ws)
    assert len(res.track_member_lattice_decode_parts(0)) == int(m[0]["n_parts"])
    # every other table of the call is that of the context without the setting
    for k in TABLES + LINKS + TRACK + LATTICE:
        assert getattr(plain, k).tobytes() == getattr(res, k).tobytes(), k
    for k in NEW:
        with pytest.raises(ValueError):
            getattr(plain, k)
    print("word tracks", len(d), "decoded", int((d["cost"] >= 0).sum()), "edits", np.bincount(d["n_edits"]).tolist(), "cut runs", int((res.run_splits["n_cuts"] > 0).sum()),
          "strings other than the track decode's", int((res.lattice_track_decode_chars != res.track_decode_chars).any(axis=1).sum()))


def test_the_setting_off_and_a_flag_missing(scene):
    S, f, frames, table, plain, res, _, _ = scene
    f.set_lattice_track_decode(False)
    try:
        off = f.text_detect_list(frames, GROUPED, **BOTH, **WANTS)
    finally:
        f.set_lattice_track_decode(True)
    for k in TABLES + LINKS + TRACK + LATTICE:
        assert getattr(plain, k).tobytes() == getattr(off, k).tobytes(), k
    for k in NEW:
        with pytest.raises(ValueError):
            getattr(off, k)
    # the setting on, either flag missing: no new table, and nothing else moves
    f.set_lattice_track_decode(False)
    a0 = f.text_detect_list(frames, GROUPED, want_track_decode=True, **WANTS)
    b0 = f.text_detect_list(frames, GROUPED, want_lattice_decode=True, **WANTS)
    f.set_lattice_track_decode(True)
    a1 = f.text_detect_list(frames, GROUPED, want_track_decode=True, **WANTS)
    b1 = f.text_detect_list(frames, GROUPED, want_lattice_decode=True, **WANTS)
    for k in TABLES + LINKS + TRACK:
        assert getattr(a0, k).tobytes() == getattr(a1, k).tobytes(), k
    for k in TABLES + LATTICE:
        assert getattr(b0, k).tobytes() == getattr(b1, k).tobytes(), k
    for r in (a1, b1):
        for k in NEW:
            with pytest.raises(ValueError):
                getattr(r, k)
    for v in (2, -1):
        assert f.L.str_er_set_lattice_track_decode(f.h, v) == -1
    again = f.text_detect_list(frames, GROUPED, **BOTH, **WANTS)          # a refused value leaves the setting on
    for k in NEW:
        assert getattr(again, k).tobytes() == getattr(res, k).tobytes(), k
    # a grouped call without lines: empty tables, not an error
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_LINKS | S.WANT_LINE_WORDS | S.WANT_RUN_READ | S.WANT_WORD_DECODE | S.WANT_RUN_SPLIT | S.WANT_TRACK_DECODE | S.WANT_LATTICE_DECODE
    blank = f.text_detect(np.full((120, 160, 3), 128, np.uint8), flags)
    assert len(blank.texts) == 0 and all(len(getattr(blank, k)) == 0 for k in NEW)


def test_a_reused_context_that_grows_and_shrinks(scene):
    S, f, frames, table, plain, res, _, _ = scene
    assert f.lattice_track_decode_stats() > 0
    few = f.text_detect_list(frames[:3], GROUPED, **BOTH, **WANTS)          # fewer words and tracks in buffers sized for more
    check_entry_point(f, few)
    assert len(few.word_track_members) < len(res.word_track_members)
    f.set_track_decode(40, 90, 1)
    f.set_run_split(1, 4, 0)
    try:
        other = f.text_detect_list(frames, GROUPED, **BOTH, **WANTS)
        check_entry_point(f, other)
        assert other.lattice_track_decodes["n_edits"].max() <= 1
    finally:
        f.set_track_decode()
        f.set_run_split()
    again = f.text_detect_list(frames, GROUPED, **BOTH, **WANTS)
    for k in NEW:
        assert getattr(again, k).tobytes() == getattr(res, k).tobytes(), k


def test_a_frame_streams_contexts_honour_the_setting(scene):
    S, f, frames, table, plain, res, path, cascade_paths = scene
    st = S.FrameStream(S.Params(max_width=640, max_height=480, max_frames=16, n_pyr_levels=3), depth=2)
    flags = GROUPED | S.WANT_MASKS | S.WANT_FRAME_LINES | S.WANT_LINE_LINKS
    wants = dict(want_line_words=True, want_run_read=True, want_word_decode=True, want_run_split=True, want_track_decode=True, want_lattice_decode=True)
    try:
        st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
        st.load_svm_model(path, 1800)
        st.set_bigram(table)
        st.set_lattice_track_decode(True)                                # (on every context of the stream)
        st.submit_copy_list(frames, flags, **wants)
        st.submit_copy_list(frames, flags, **wants)
        for _ in range(2):
            _, got = st.next()
            for k in NEW + TRACK + LATTICE:
                assert getattr(got, k).tobytes() == getattr(res, k).tobytes(), k
        st.set_lattice_track_decode(False)
        st.submit_copy_list(frames, flags, **wants)
        _, got = st.next()
        for k in NEW:
            with pytest.raises(ValueError):
                getattr(got, k)
        for k in TRACK + LATTICE:
            assert getattr(got, k).tobytes() == getattr(res, k).tobytes(), k
    finally:
        st.close()
