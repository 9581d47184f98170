"""WordTracker and the track pool behind the detect calls, with the fixture of test_track_read_pipeline.py (the shipped model, make_video,
the lexicon built from the readings).  A static video -- one frame six times -- through calls of 2 + 2 + 2 and of 3 + 3 frames: the
persistent word tracks are the word tracks of the one call of six frames and their pooled records its track matches, for a pool of rows,
beside STR_ER_WANT_RUN_SPLIT and for a lattice pool.  The moving video in calls of four frames against a numpy statement of the update
rules (word_tracker_ref.py), through list calls and through a FrameStream; a pool that is too small."""
import numpy as np
import pytest

import word_match_ref as WM
from test_frame_lines import GROUPED
from test_track_read_pipeline import WANTS, scene  # noqa: F401  (the fixture)
from word_tracker_ref import WordTrackerRef

pytestmark = pytest.mark.gpu
SEVEN = ("entry", "cost", "second_entry", "second_cost", "free_cost", "n_tried", "n_used")
MODES = {"rows": dict(), "split": dict(want_run_split=True), "lattice": dict(want_run_split=True)}


def seven(rec):
    return tuple(int(rec[k]) for k in SEVEN)


@pytest.mark.parametrize("mode", list(MODES))
def test_static_video_in_calls_of_two_and_of_three_frames(scene, mode):  # noqa: F811
    S, f, prm, path, frames, seg_of, lexicon, plain, res = scene
    still = [frames[0]] * 6
    extra = dict(want_lattice_match=True, want_lattice_track=True) if mode == "lattice" else {}
    one = f.text_detect_list(still, GROUPED, want_track_read=True, **WANTS, **MODES[mode], **extra)
    want = one.lattice_track_matches if mode == "lattice" else one.track_matches
    tracks, of = one.word_tracks, one.word_track_of_words
    assert len(tracks) >= 2, "the frame gives fewer than two word tracks: choose another frame"
    assert ((tracks["first_frame"] == 0) & (tracks["last_frame"] == 5)).any(), "no word track has members from all three calls: choose another frame"
    for cuts in ((0, 2, 4, 6), (0, 3, 6)):
        pool = S.TrackPool(f, 4 * len(tracks), lattice=mode == "lattice")
        try:
            tracker = S.WordTracker(f, pool)
            ids, boxes = [], []
            for lo, hi in zip(cuts, cuts[1:]):
                part = f.text_detect_list(still[lo:hi], GROUPED, want_track_read=True, **WANTS, **MODES[mode])
                ids.append(tracker.update(part))
                boxes.append(part.words[["x", "y", "w", "h"]].tolist())
            assert sum(boxes, []) == one.words[["x", "y", "w", "h"]].tolist()          # (the same words, in the same order)
            ids = tracker.resolve(np.concatenate(ids))
            fwd, back = {}, {}
            for i, t in zip(ids.tolist(), of.tolist()):                                 # every word's persistent track has the members of the one call's
                assert (i < 0) == (t < 0)
                if t >= 0:
                    assert fwd.setdefault(i, t) == t and back.setdefault(t, i) == i, (i, t)
            assert len(back) == len(tracks)
            recs = tracker.read([back[t] for t in range(len(tracks))])
            for t in range(len(tracks)):
                assert seven(recs[t]) == seven(want[t]) and int(recs[t]["n_members"]) == int(tracks[t]["count"]), (t, recs[t], want[t])
                e = int(want[t]["entry"])
                assert tracker.text(back[t]) == (lexicon[e] if e >= 0 else None)
            done = {i for i, _ in tracker.closed}
            assert all((back[t] in done) == (int(tracks[t]["last_frame"]) < 5) for t in range(len(tracks)))
            tracker.reset()                                                             # a known cut: everything is closed, the pool is free again
            assert pool.info()["in_use"] == 0 and {i for i, _ in tracker.closed} == set(back.values())
            assert [seven(r) for r in tracker.read([back[t] for t in range(len(tracks))])] == [seven(want[t]) for t in range(len(tracks))]
        finally:
            pool.close()


def _ref_tables(part, lexicon):
    first, last = part.edge_feet(0), part.edge_feet(1)
    return (part.words, part.word_track_of_words, part.word_tracks, part.word_track_members, (part.run_costs, part.words["first_run"], part.words["n_runs"]), first.lines,
            last.lines, (first.width, first.height), (last.width, last.height))


def _moving(scene, results):  # noqa: F811
    """WordTracker over `results` against the reference; returns (ids per result, records of all ids, closed, the final id of every id)."""
    S, f, prm, path, frames, seg_of, lexicon, plain, res = scene
    pool = S.TrackPool(f, 256)
    try:
        tracker, lines = S.WordTracker(f, pool), S.TextTracker(f)
        ref = WordTrackerRef(WM.Lexicon(lexicon, True))
        ids = []
        for part in results:
            tids = lines.update(part)
            want = ref.update(*_ref_tables(part, lexicon), tids, lines.resolve)
            got = tracker.update(part)
            assert got.tolist() == want.tolist()
            assert [(i, tuple(int(v) for v in r)) for i, r in tracker.closed] == ref.closed
            live = sorted(ref.live)
            assert sorted(tracker._slot) == live and [tuple(int(v) for v in r) for r in tracker.read(live)] == [ref.record(i) for i in live]
            ids.append(got)
        every = list(range(len(ref.parent)))
        assert tracker.resolve(every).tolist() == [ref.find(i) for i in every]
        return ids, [tuple(int(v) for v in r) for r in tracker.read(every)], list(ref.closed), [ref.find(i) for i in every]
    finally:
        pool.close()


@pytest.fixture(scope="module")
def moving(scene):  # noqa: F811
    S, f, prm, path, frames, seg_of, lexicon, plain, res = scene
    n12 = sum(s < 2 for s in seg_of)                          # the first part of one size: twelve frames with a cut in the middle
    parts = [f.text_detect_list(frames[lo:lo + 4], GROUPED, want_track_read=True, **WANTS) for lo in range(0, n12, 4)]
    return parts, _moving(scene, parts)


def test_moving_video_in_calls_of_four_frames(scene, moving):  # noqa: F811
    S, f, prm, path, frames, seg_of, lexicon, plain, res = scene
    parts, (ids, records, closed, root) = moving
    cut = seg_of.index(1)                                     # the first frame behind the cut
    frames_of = {}
    for k, (part, got) in enumerate(zip(parts, ids)):
        fr = part.texts["frame"][part.words["line"]].astype(int) + 4 * k
        for i, g in zip(got.tolist(), fr.tolist()):
            if i >= 0:
                frames_of.setdefault(root[i], set()).add(g)          # (an id handed out earlier may have been joined since: its final id counts)
    assert any(len({g // 4 for g in fs}) >= 2 for fs in frames_of.values()), "no id spans two calls: change the motion"
    assert not any(min(fs) < cut <= max(fs) for fs in frames_of.values()), "a persistent track across the cut"
    ended = {i for i, fs in frames_of.items() if max(fs) < 11}
    assert ended and ended <= {i for i, _ in closed} and all(records[i][7] >= len(frames_of[i]) for i in frames_of)


def test_the_same_calls_through_a_stream(scene, moving, cascade_paths):  # noqa: F811
    S, f, prm, path, frames, seg_of, lexicon, plain, res = scene
    parts, want = moving
    st = S.FrameStream(prm, depth=2)
    try:
        st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
        st.load_svm_model(path, 1800)
        st.set_lexicon(lexicon)
        st.set_word_link(1, 2)
        got = []
        for lo in range(0, 4 * len(parts), 4):
            slot, buf = st.acquire()
            layout, off = [], 0
            for fr in frames[lo:lo + 4]:
                h, w = fr.shape[:2]
                buf[off:off + 3 * w * h] = fr.reshape(-1)
                layout.append((off, w, h, 3 * w))
                off += (3 * w * h + 255) // 256 * 256
            st.submit_list(slot, layout, GROUPED | S.WANT_MASKS | S.WANT_FRAME_LINES | S.WANT_LINE_LINKS, want_line_words=True, want_run_read=True, want_word_match=True,
                           want_track_read=True)
            got.append(st.next()[1])
        ids, records, closed, root = _moving(scene, got)
        assert [a.tolist() for a in ids] == [a.tolist() for a in want[0]] and records == want[1] and closed == want[2] and root == want[3]
    finally:
        st.close()


def test_a_pool_that_is_too_small(scene, moving):  # noqa: F811
    S, f, prm, path, frames, seg_of, lexicon, plain, res = scene
    parts, _ = moving
    assert len(parts[0].word_tracks) > 2
    pool = S.TrackPool(f, 2)
    try:
        tracker = S.WordTracker(f, pool)
        with pytest.raises(S.StrErError) as e:
            tracker.update(parts[0])
        assert e.value.code == -7
        assert tracker._parent == [] and tracker.closed == [] and tracker._prev is None and sorted(tracker._free) == [0, 1] and pool.info()["in_use"] == 0
        tracker.reset()
        blank = f.text_detect(np.full((120, 160, 3), 128, np.uint8), GROUPED, want_track_read=True, **WANTS)
        assert len(tracker.update(blank)) == 0 and tracker.closed == []
    finally:
        pool.close()
