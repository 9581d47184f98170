"""STR_ER_WANT_TRACK_READ in the detect calls, on the 16-frame video of test_line_links.py (a cut, a change of size) with the shipped
model: from the call's own tables -- line_feet, line_tracks, words, run_costs -- the reference (track_read_ref.py) gives every new
table, compared with ==; the other tables are byte for byte those of the call without the flag; the same through a batch call, a
stream submission, another link threshold and beside STR_ER_WANT_RUN_SPLIT.  The frames hold box glyphs, not rendered words: the
lexicon is what the runs of the words read, a few of those strings changed, and random distractors."""
import numpy as np
import pytest

import track_read_ref as TR
import word_match_ref as WM
from test_frame_lines import GROUPED, _same
from test_line_links import make_video
from test_svm_exact import _shipped

pytestmark = pytest.mark.gpu
TABLES = ("line_words", "line_runs", "words", "run_reads", "run_features", "line_feet", "line_pairs", "frame_lines", "frame_line_members", "masks", "mask_bits",
          "line_links", "line_tracks", "text_tracks", "text_track_members", "word_matches", "run_costs", "run_probs")
NEW = ("word_links", "word_tracks", "word_track_members", "word_track_of_words", "track_matches", "track_member_costs")
WANTS = dict(want_masks=True, want_frame_lines=True, want_line_links=True, want_line_words=True, want_run_read=True, want_word_match=True)


@pytest.fixture(scope="module")
def scene(S, cascade_paths, tmp_path_factory):
    path, m = _shipped(S, tmp_path_factory, 5)
    prm = S.Params(max_width=640, max_height=480, max_frames=16, n_pyr_levels=3)
    f = S.ERFilter(params=prm)
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    f.load_svm_model(path, 1800)
    frames, seg_of = make_video(S)
    first = f.text_detect_list(frames, GROUPED, want_frame_lines=True, want_line_words=True, want_run_read=True)
    rng = np.random.default_rng(9)
    read = sorted({first.word_text(w) for w in range(len(first.words))})
    read = [t for t in read if 1 <= len(t) <= 32]
    near = [t[:-1] for t in read if len(t) > 2][:40] + [t[:1] + "Z" + t[2:] for t in read if len(t) > 2][:40] + [t.swapcase() for t in read][:40]
    lexicon = read + near + ["".join(rng.choice(list(WM.ALPHABET), int(rng.integers(1, 13)))) for _ in range(300)]
    f.set_lexicon(lexicon)
    plain = f.text_detect_list(frames, GROUPED, **WANTS)
    res = f.text_detect_list(frames, GROUPED, want_track_read=True, **WANTS)
    yield S, f, prm, path, frames, seg_of, lexicon, plain, res
    f.close()


def reference(res, sizes, lexicon, num=1, den=2, rows=None, fold=True):
    """Every new table from the result's own feet, tracks, words and cost rows.  rows: (costs, first, n) where they are not the runs'."""
    frames = res.texts["frame"].astype(np.uint32)
    reading, links = TR.word_links(res.line_feet["pixels"], frames, res.line_tracks, sizes, res.words, num, den)
    track_of, tracks, members = TR.word_tracks(frames, res.line_tracks, reading, res.words, links)
    costs, first, n_of = rows if rows is not None else (res.run_costs, res.words["first_run"], res.words["n_runs"])
    matches, mc = TR.match_tracks(costs, first, n_of, [t["first"] for t in tracks], [t["count"] for t in tracks], members, WM.Lexicon(lexicon, fold))
    return reading, links, track_of, tracks, members, matches, mc


def check(res, ref):
    reading, links, track_of, tracks, members, matches, mc = ref
    assert [tuple(int(l[k]) for k in ("a", "b", "inter", "link")) for l in res.word_links] == links
    assert res.word_track_of_words.tolist() == track_of.tolist() and len(track_of) == len(res.words)
    assert TR.tracks_as_dicts(res.word_tracks) == tracks
    assert res.word_track_members.tolist() == members.tolist()
    assert TR.as_tuples(res.track_matches) == matches
    assert res.track_member_costs.tolist() == mc.tolist()


def test_list_call_against_the_reference(scene):
    S, f, prm, path, frames, seg_of, lexicon, plain, res = scene
    sizes = [(fr.shape[1], fr.shape[0]) for fr in frames]
    ref = reference(res, sizes, lexicon)
    reading, links, track_of, tracks, members, matches, mc = ref
    # the video must give the reference something to decide
    frame_of_word = res.texts["frame"][res.words["line"]]
    spans = [len({int(frame_of_word[w]) for w in members[t["first"]:t["first"] + t["count"]]}) for t in tracks]
    assert max(spans + [0]) >= 4, "no word track has members in four frames: change the motion or the seed"
    assert (track_of < 0).any(), "every word is eligible: change the motion or the seed"
    per_text = np.bincount([t["text_track"] for t in tracks])
    assert (per_text >= 2).any(), "no text track holds two word tracks: change the motion or the seed"
    change = [i for i in range(1, len(seg_of)) if seg_of[i] != seg_of[i - 1]]          # the first frames after the cut and after the change of size
    assert len(links) > 0 and not any(int(frame_of_word[b]) in change for a, b, _, _ in links), "a word link across the cut or the change of size"
    assert any(int(frame_of_word[w]) == c - 1 for c in change for w in range(len(res.words)) if track_of[w] >= 0), "no eligible word before a cut: change the seed"
    check(res, ref)
    # every other table is that of the call without the flag
    for k in NEW:
        with pytest.raises(ValueError):
            getattr(plain, k)
    _same(plain, res)
    for k in TABLES:
        assert getattr(plain, k).tobytes() == getattr(res, k).tobytes(), k
    # the entry point on the result's cost rows and members
    tm, mc2 = f.match_tracks(res.run_costs, res.words["first_run"], res.words["n_runs"], res.word_tracks["first"], res.word_tracks["count"], res.word_track_members)
    assert tm.tobytes() == res.track_matches.tobytes() and mc2.tobytes() == res.track_member_costs.tobytes()
    # the texts
    for g in range(len(res.word_tracks)):
        e = int(res.track_matches[g]["entry"])
        assert res.word_track_text(g) == (lexicon[e] if e >= 0 else res.word_text(int(res.word_tracks[g]["rep"])))
    for k, t in enumerate(res.text_tracks):
        lw = res.line_words[int(t["rep"])]
        ws = range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))
        assert res.text_track_match_text(k) == " ".join(res.word_track_text(int(track_of[w])) if track_of[w] >= 0 else res.word_text(w) for w in ws)
    differ = sum(any(int(res.word_matches[w]["entry"]) != int(m[0]) for w in members[t["first"]:t["first"] + t["count"]]) for t, m in zip(tracks, matches))
    print("word tracks", len(tracks), "longest", max(spans + [0]), "frames; tracks whose entry differs from some member's own:", differ)


def test_another_threshold_and_a_batch_call(scene):
    S, f, prm, path, frames, seg_of, lexicon, plain, res = scene
    sizes = [(fr.shape[1], fr.shape[0]) for fr in frames]
    f.set_word_link(9, 10)
    try:
        stiff = f.text_detect_list(frames, GROUPED, want_track_read=True, **WANTS)
        ref = reference(stiff, sizes, lexicon, 9, 10)
        assert any(link == 0 for _, _, _, link in ref[1]), "every overlap is a link at 9 / 10: change the motion"
        check(stiff, ref)
        assert len(stiff.word_tracks) > len(res.word_tracks)
    finally:
        f.set_word_link()
    n12 = sum(s < 2 for s in seg_of)                          # the equal-size part as one batch call
    batch = f.text_detect(np.stack(frames[:n12]), GROUPED, want_track_read=True, **WANTS)
    check(batch, reference(batch, sizes[:n12], lexicon))
    assert len(batch.word_tracks) > 0


def test_stream_submission(scene, cascade_paths):
    S, f, prm, path, frames, seg_of, lexicon, plain, res = scene
    st = S.FrameStream(prm, depth=2)
    try:
        st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
        st.load_svm_model(path, 1800)
        st.set_lexicon(lexicon)
        st.set_word_link(1, 2)
        slot, buf = st.acquire()
        layout, off = [], 0
        for fr in frames:
            h, w = fr.shape[:2]
            buf[off:off + 3 * w * h] = fr.reshape(-1)
            layout.append((off, w, h, 3 * w))
            off += (3 * w * h + 255) // 256 * 256
        st.submit_list(slot, layout, GROUPED | S.WANT_MASKS | S.WANT_FRAME_LINES | S.WANT_LINE_LINKS, want_line_words=True, want_run_read=True, want_word_match=True,
                       want_track_read=True)
        _, a = st.next()
        for k in TABLES + NEW:
            assert getattr(a, k).tobytes() == getattr(res, k).tobytes(), k
        assert [a.word_track_text(g) for g in range(len(a.word_tracks))] == [res.word_track_text(g) for g in range(len(res.word_tracks))]
    finally:
        st.close()


def test_beside_the_run_split(scene):
    S, f, prm, path, frames, seg_of, lexicon, plain, res = scene
    sizes = [(fr.shape[1], fr.shape[0]) for fr in frames]
    split = f.text_detect_list(frames, GROUPED, want_run_split=True, want_track_read=True, **WANTS)
    rows = np.array([split.run_costs[int(p["run"])] if int(p["piece"]) < 0 else split.piece_costs[int(p["piece"])] for p in split.split_parts],
                    np.uint8).reshape(-1, 65)
    check(split, reference(split, sizes, lexicon, rows=(rows, split.word_splits["first_part"], split.word_splits["n_parts"])))
    for k in NEW[:4]:                                         # the links and the tracks are those of the words: the split moves none
        assert getattr(split, k).tobytes() == getattr(res, k).tobytes(), k
    alone = f.text_detect_list(frames, GROUPED, want_run_split=True, **WANTS)
    for k in TABLES + ("run_splits", "run_pieces", "piece_reads", "piece_costs", "split_parts", "word_splits"):
        assert getattr(alone, k).tobytes() == getattr(split, k).tobytes(), k


def test_flag_rules_leave_the_context_usable(scene):
    S, f, prm, path, frames, seg_of, lexicon, plain, res = scene
    two = np.stack(frames[:2])
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS | S.WANT_RUN_READ
    with pytest.raises(S.StrErError) as e:                    # without STR_ER_WANT_LINE_LINKS
        f.text_detect(two, flags | S.WANT_WORD_MATCH | S.WANT_TRACK_READ)
    assert e.value.code == -1 and "STR_ER_WANT_TRACK_READ" in str(e.value)
    with pytest.raises(S.StrErError) as e:                    # without STR_ER_WANT_WORD_MATCH
        f.text_detect(two, flags | S.WANT_LINE_LINKS | S.WANT_TRACK_READ)
    assert e.value.code == -1 and "STR_ER_WANT_TRACK_READ" in str(e.value)
    planes = f.compute_channels(frames[0])
    with pytest.raises(S.StrErError) as e:                    # the per-plane calls
        f.detect_planes(planes[:1], S.STAGE_ALL | S.WANT_FRAME_LINES | S.WANT_LINE_LINKS | S.WANT_LINE_WORDS | S.WANT_RUN_READ | S.WANT_WORD_MATCH | S.WANT_TRACK_READ)
    assert e.value.code == -1 and "STR_ER_WANT_TRACK_READ" in str(e.value)
    # a grouped call without lines: empty tables, not an error
    blank = f.text_detect(np.full((120, 160, 3), 128, np.uint8), flags | S.WANT_LINE_LINKS | S.WANT_WORD_MATCH | S.WANT_TRACK_READ)
    assert len(blank.texts) == 0 and all(len(getattr(blank, k)) == 0 for k in NEW)
    good = f.text_detect_list(frames, GROUPED, want_track_read=True, **WANTS)
    for k in NEW:
        assert getattr(good, k).tobytes() == getattr(res, k).tobytes(), k
