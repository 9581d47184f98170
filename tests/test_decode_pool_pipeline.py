"""WordTracker and the decode pool behind the detect calls, with the fixture of test_track_decode_pipeline.py (the shipped model,
make_video, a bigram table built from the readings, no lexicon set).  A static video -- one frame six times -- through calls of 2 + 2 + 2
and of 3 + 3 frames: the persistent word tracks are the word tracks of the one call of six frames, and their pooled records, labels and
member costs that call's track decodes.  The moving video in calls of four frames against a numpy statement of the update rules with
kept lists (decode_tracker_ref.py, on top of word_tracker_ref.py).  Both pools at once: the lexicon side is byte for byte that of
WordTracker(f, pool) alone.  A result whose rows a folding lexicon folded is refused before either pool is touched."""
import numpy as np
import pytest

import decode_pool_ref as DP
from decode_tracker_ref import DecodeTrackerRef
from test_frame_lines import GROUPED
from test_track_decode_pipeline import WANTS, scene  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
EIGHT = DP.FIELDS[:8]


def test_static_video_in_calls_of_two_and_of_three_frames(scene):  # noqa: F811
    S, f, frames, read, table, plain, res = scene
    still = [frames[0]] * 6
    one = f.text_detect_list(still, GROUPED, want_track_decode=True, **WANTS)
    tracks, of, members, n_runs = one.word_tracks, one.word_track_of_words, one.word_track_members, one.words["n_runs"]
    assert len(tracks) >= 2, "the frame gives fewer than two word tracks: choose another frame"
    assert ((tracks["first_frame"] == 0) & (tracks["last_frame"] == 5)).any(), "no word track has members from all three calls: choose another frame"
    for cuts in ((0, 2, 4, 6), (0, 3, 6)):
        pool = S.DecodePool(f, 256, keep=8)
        try:
            tracker = S.WordTracker(f, decode_pool=pool)
            ids, boxes = [], []
            for lo, hi in zip(cuts, cuts[1:]):
                part = f.text_detect_list(still[lo:hi], GROUPED, want_track_decode=True, **WANTS)
                ids.append(tracker.update(part))
                boxes.append(part.words[["x", "y", "w", "h"]].tolist())
            assert sum(boxes, []) == one.words[["x", "y", "w", "h"]].tolist()          # (the same words, in the same order)
            ids = tracker.resolve(np.concatenate(ids))
            fwd, back = {}, {}
            for i, t in zip(ids.tolist(), of.tolist()):
                assert (i < 0) == (t < 0)
                if t >= 0:
                    assert fwd.setdefault(i, t) == t and back.setdefault(t, i) == i, (i, t)
            assert len(back) == len(tracks)
            recs, chars = tracker.read_decode([back[t] for t in range(len(tracks))])
            for t in range(len(tracks)):
                want, mine = one.track_decodes[t], [int(w) for w in members[int(tracks[t]["first"]):int(tracks[t]["first"]) + int(tracks[t]["count"])]]
                usable = [j for j, w in enumerate(mine) if n_runs[w] <= 32]
                assert len(usable) <= 6                                                 # (keep = 8: the kept list is the call's member list, in its order)
                assert [int(recs[t][k]) for k in EIGHT if k != "seed_member"] == [int(want[k]) for k in EIGHT if k != "seed_member"], (t, recs[t], want)
                assert (int(recs[t]["n_members"]), int(recs[t]["n_kept"])) == (len(mine), len(usable))
                rank = int(recs[t]["seed_member"])
                assert (rank < 0 and int(want["seed_member"]) < 0) or mine[usable[rank]] == int(want["seed_member"])
                assert chars[t].tolist() == one.track_decode_chars[t].tolist()
                assert tracker.decode_text(back[t]) == (one.word_track_decode_text(t) if int(want["cost"]) >= 0 else None)
                if back[t] in tracker._slot:                                            # a live track: its member costs, in age order
                    _, _, mc = pool.read([tracker._slot[back[t]]])
                    own = one.track_decode_member_costs[int(tracks[t]["first"]):int(tracks[t]["first"]) + int(tracks[t]["count"])]
                    assert mc[0][:len(usable)].tolist() == [int(own[j]) for j in usable] and (mc[0][len(usable):] == -1).all()
            done = {i for i, _, _ in tracker.closed_decodes}
            assert all((back[t] in done) == (int(tracks[t]["last_frame"]) < 5) for t in range(len(tracks))) and tracker.closed == []
            with pytest.raises(ValueError):
                tracker.read([back[0]])
            tracker.reset()                                                             # a known cut: everything is closed, the pool is free again
            assert pool.info()["in_use"] == 0 and {i for i, _, _ in tracker.closed_decodes} == set(back.values())
            again, chars2 = tracker.read_decode([back[t] for t in range(len(tracks))])
            assert again.tobytes() == recs.tobytes() and chars2.tobytes() == chars.tobytes()
        finally:
            pool.close()


def _ref_tables(part):
    first, last = part.edge_feet(0), part.edge_feet(1)
    return (part.words, part.word_track_of_words, part.word_tracks, part.word_track_members, (part.run_costs, part.words["first_run"], part.words["n_runs"]), first.lines,
            last.lines, (first.width, first.height), (last.width, last.height))


def _flat(rec, chars):
    return tuple(int(rec[k]) for k in DP.FIELDS), tuple(int(a) for a in chars)


@pytest.fixture(scope="module")
def parts(scene):  # noqa: F811
    S, f, frames, read, table, plain, res = scene
    from test_line_links import make_video
    seg_of = make_video(S)[1]
    n12 = sum(s < 2 for s in seg_of)                          # the first part of one size: twelve frames with a cut in the middle
    return [f.text_detect_list(frames[lo:lo + 4], GROUPED, want_track_decode=True, **WANTS) for lo in range(0, n12, 4)], seg_of


@pytest.mark.parametrize("keep", [3, 32])
def test_moving_video_in_calls_of_four_frames(scene, parts, keep):  # noqa: F811
    S, f, frames, read, table, plain, res = scene
    parts, seg_of = parts
    pool = S.DecodePool(f, 256, keep=keep)
    try:
        tracker, lines = S.WordTracker(f, decode_pool=pool), S.TextTracker(f)
        ref = DecodeTrackerRef(S, table, keep)
        spans = []
        for part in parts:
            tids = lines.update(part)
            want = ref.update(*_ref_tables(part), tids, lines.resolve)
            got = tracker.update(part)
            assert got.tolist() == want.tolist()
            assert [(i, _flat(r, ch)) for i, r, ch in tracker.closed_decodes] == ref.closed
            live = sorted(ref.live)
            recs, chars = tracker.read_decode(live)
            assert sorted(tracker._slot) == live and [_flat(r, ch) for r, ch in zip(recs, chars)] == [ref.record(i) for i in live]
            spans.append(recs["n_members"].max() if len(recs) else 0)
        every = list(range(len(ref.parent)))
        assert tracker.resolve(every).tolist() == [ref.find(i) for i in every]
        assert max(spans) > 4, "no id spans two calls: change the motion"
        ended = [i for i, _ in ref.closed]
        assert ended and all(tracker.decode_text(i) == ("".join(S.ocr_char(a) for a in ch[:rec[2]]) if rec[0] >= 0 else None) for i, (rec, ch) in ref.closed[:8])
        if keep == 3:
            assert any(rec[8] > rec[9] == 3 for _, (rec, _) in ref.closed), "nothing was evicted: choose a smaller keep"
    finally:
        pool.close()


def test_both_pools_at_once(scene, parts):  # noqa: F811
    S, f, frames, read, table, plain, res = scene
    n = 4 * len(parts[0])
    f.set_lexicon(read, fold_case=False)
    wants = dict(WANTS, want_word_match=True, want_track_read=True, want_track_decode=True)
    pools = [S.TrackPool(f, 256), S.TrackPool(f, 256), S.DecodePool(f, 256, keep=8), S.DecodePool(f, 300, keep=8)]
    try:
        alone, beside, decode = S.WordTracker(f, pools[0]), S.WordTracker(f, pools[1], pools[2]), S.WordTracker(f, decode_pool=pools[3])
        for lo in range(0, n, 4):
            part = f.text_detect_list(frames[lo:lo + 4], GROUPED, **wants)
            ids = [t.update(part).tolist() for t in (alone, beside, decode)]
            assert ids[0] == ids[1] == ids[2] and alone._slot == beside._slot == decode._slot and alone._free == beside._free
        every = list(range(len(alone._parent)))
        assert len(every) > 0 and beside.read(every).tobytes() == alone.read(every).tobytes()          # the lexicon side: byte for byte
        assert [(i, r.tobytes()) for i, r in beside.closed] == [(i, r.tobytes()) for i, r in alone.closed] and len(alone.closed) > 0
        assert all(a.tobytes() == b.tobytes() for a, b in zip(beside.read_decode(every), decode.read_decode(every)))
        assert [(i, r.tobytes(), c.tobytes()) for i, r, c in beside.closed_decodes] == [(i, r.tobytes(), c.tobytes()) for i, r, c in decode.closed_decodes]
        assert [i for i, _ in beside.closed] == [i for i, _, _ in beside.closed_decodes]
        assert pools[1].info()["in_use"] == pools[2].info()["in_use"] == pools[0].info()["in_use"]
        with pytest.raises(ValueError):
            decode.read(every[:1])
        with pytest.raises(ValueError):
            alone.read_decode(every[:1])
        with pytest.raises(ValueError):
            S.WordTracker(f)
    finally:
        for p in pools:
            p.close()
        f.set_lexicon([])


def test_a_folded_result_is_refused_before_either_pool_is_touched(scene):  # noqa: F811
    S, f, frames, read, table, plain, res = scene
    f.set_lexicon(read)                                       # fold_case: with want_word_match the result's run_costs are folded
    pools = [S.TrackPool(f, 64), S.DecodePool(f, 64, keep=4)]
    try:
        part = f.text_detect_list(frames[:2], GROUPED, **dict(WANTS, want_word_match=True, want_track_read=True, want_track_decode=True))
        assert len(part.word_tracks) > 0
        tracker = S.WordTracker(f, pools[0], pools[1])
        with pytest.raises(ValueError, match="folded"):
            tracker.update(part)
        assert tracker._parent == [] and tracker._prev is None and len(tracker._free) == 64 and pools[0].info()["in_use"] == pools[1].info()["in_use"] == 0
        assert S.WordTracker(f, pools[0]).update(part).shape == (len(part.words),)          # the lexicon pool alone takes it, as before
    finally:
        for p in pools:
            p.close()
        f.set_lexicon([])
