"""WordTracker and the lattice decode pool behind the detect calls, with the fixture of test_track_decode_pipeline.py (the shipped model,
make_video, a bigram table built from the readings, no lexicon set) and the calls made with want_run_split, want_word_decode,
want_track_decode and want_lattice_decode.  A static video -- one frame six times -- through calls of 2 + 2 + 2 and of 3 + 3 frames:
every live and closed id's record and labels are those of str_er_lattice_decode_tracks_host on the concatenation of its members over
the calls, which is the member list of the one call of six frames -- with keep = 8 all of it, with keep = 2 its newest two usable
members, the older ones evicted across the calls.  One call with keep >= the history equals that call's
lattice_track_decodes.  A lexicon lattice pool and the new pool at once give what each gives alone.  A result whose rows a folding
lexicon folded is refused before either pool is touched."""
import numpy as np
import pytest

import lattice_decode_pool_ref as LP
from test_frame_lines import GROUPED
from test_track_decode_pipeline import WANTS, scene  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
EIGHT = LP.FIELDS[:8]
LWANTS = dict(WANTS, want_run_split=True, want_track_decode=True, want_lattice_decode=True)


def _tables(r):
    return r.run_splits, r.run_costs, r.piece_costs, r.words["first_run"], r.words["n_runs"]


def _nodes(r, w):
    f, n = int(r.words["first_run"][w]), int(r.words["n_runs"][w])
    return int((r.run_splits["n_cuts"][f:f + n] + 1).sum())


@pytest.fixture(scope="module")
def still(scene):  # noqa: F811
    S, f, frames, read, table, plain, res = scene
    six = [frames[0]] * 6
    f.set_lattice_track_decode(True)
    try:
        one = f.text_detect_list(six, GROUPED, **LWANTS)
    finally:
        f.set_lattice_track_decode(False)
    assert len(one.word_tracks) >= 2, "the frame gives fewer than two word tracks: choose another frame"
    return six, one


def test_static_video_in_calls_of_two_and_of_three_frames(scene, still):  # noqa: F811
    S, f, frames, read, table, plain, res = scene
    six, one = still
    tracks, of, members = one.word_tracks, one.word_track_of_words, one.word_track_members
    assert ((tracks["first_frame"] == 0) & (tracks["last_frame"] == 5)).any(), "no word track has members from all three calls: choose another frame"
    # the host on the one call's tables: every track's members are the concatenation of its members over the shorter calls
    host, hch = S.lattice_decode_tracks_host(*_tables(one), tracks["first"], tracks["count"], members, table)[:2]
    assert host.tobytes() == one.lattice_track_decodes.tobytes() and hch.tobytes() == one.lattice_track_decode_chars.tobytes()
    lists = [[int(w) for w in members[int(t["first"]):int(t["first"]) + int(t["count"])]] for t in tracks]
    usable_of = [[j for j, w in enumerate(mine) if _nodes(one, w) <= 32] for mine in lists]
    assert max(len(u) for u in usable_of) > 2, "no track has more than two usable members: keep = 2 evicts nothing"
    for cuts, keep in (((0, 2, 4, 6), 8), ((0, 3, 6), 8), ((0, 2, 4, 6), 2), ((0, 3, 6), 2)):
        # the newest `keep` usable members of every track, as tracks of their own for the host
        kept_of = [[mine[j] for j in u[-keep:]] for mine, u in zip(lists, usable_of)]
        kf = np.concatenate([[0], np.cumsum([len(k) for k in kept_of])[:-1]]).astype(np.int32)
        host, hch = S.lattice_decode_tracks_host(*_tables(one), kf, np.array([len(k) for k in kept_of], np.int32), np.array(sum(kept_of, []), np.int32), table)[:2]
        if keep == 8:
            assert [int(h["cost"]) for h in host] == [int(h["cost"]) for h in one.lattice_track_decodes]
        pool = S.LatticeDecodePool(f, 256, keep=keep)
        try:
            tracker = S.WordTracker(f, decode_pool=pool)
            ids, boxes = [], []
            for lo, hi in zip(cuts, cuts[1:]):
                part = f.text_detect_list(six[lo:hi], GROUPED, **LWANTS)
                ids.append(tracker.update(part))
                boxes.append(part.words[["x", "y", "w", "h"]].tolist())
            assert sum(boxes, []) == one.words[["x", "y", "w", "h"]].tolist()          # (the same words, in the same order)
            ids = tracker.resolve(np.concatenate(ids))
            back = {}
            for i, t in zip(ids.tolist(), of.tolist()):
                assert (i < 0) == (t < 0)
                if t >= 0:
                    assert back.setdefault(t, i) == i, (i, t)
            assert len(back) == len(tracks)
            recs, chars = tracker.read_decode([back[t] for t in range(len(tracks))])
            for t in range(len(tracks)):
                want, mine, kept = host[t], lists[t], kept_of[t]
                assert len(usable_of[t]) <= 6                                           # (keep = 8: the kept list is the call's member list, in its order)
                assert [int(recs[t][k]) for k in EIGHT if k != "seed_member"] == [int(want[k]) for k in EIGHT if k != "seed_member"], (t, recs[t], want)
                assert (int(recs[t]["n_members"]), int(recs[t]["n_kept"])) == (len(mine), len(kept))
                rank = int(recs[t]["seed_member"])
                assert (rank < 0 and int(want["seed_member"]) < 0) or kept[rank] == int(want["seed_member"])
                assert chars[t].tolist() == hch[t].tolist()
            done = {i for i, _, _ in tracker.closed_decodes}
            assert all((back[t] in done) == (int(tracks[t]["last_frame"]) < 5) for t in range(len(tracks))) and tracker.closed == []
            tracker.reset()                                                             # a known cut: everything is closed, the pool is free again
            assert pool.info()["in_use"] == 0 and {i for i, _, _ in tracker.closed_decodes} == set(back.values())
            again, chars2 = tracker.read_decode([back[t] for t in range(len(tracks))])
            assert again.tobytes() == recs.tobytes() and chars2.tobytes() == chars.tobytes()
        finally:
            pool.close()


def test_one_call_with_keep_past_the_history_is_that_calls_decode(scene, still):  # noqa: F811
    S, f, frames, read, table, plain, res = scene
    six, one = still
    tracks, members = one.word_tracks, one.word_track_members
    pool = S.LatticeDecodePool(f, 256, keep=8)
    try:
        tracker = S.WordTracker(f, decode_pool=pool)
        ids = tracker.update(one)
        live = sorted(tracker._slot)
        slot_of = {int(one.word_track_of_words[w]): tracker._slot[int(i)] for w, i in enumerate(ids.tolist()) if i >= 0 and int(i) in tracker._slot}
        assert len(slot_of) == len(live) > 0
        for t, slot in slot_of.items():
            rec, ch, mc, mrec, src, parts = pool.read_lattice([slot])
            want = one.lattice_track_decodes[t]
            lo, n = int(tracks[t]["first"]), int(tracks[t]["count"])
            usable = [j for j in range(n) if _nodes(one, int(members[lo + j])) <= 32]
            assert [int(rec[0][k]) for k in EIGHT if k != "seed_member"] == [int(want[k]) for k in EIGHT if k != "seed_member"]
            assert ch[0].tobytes() == one.lattice_track_decode_chars[t].tobytes()
            own = one.lattice_track_decode_members[[lo + j for j in usable]]
            for k in ("cost", "n_parts", "n_del", "n_ins"):
                assert mrec[0][:len(usable)][k].tolist() == own[k].tolist()
            assert mrec[0][:len(usable)]["word"].tolist() == list(range(len(usable))) and mc[0][:len(usable)].tolist() == own["cost"].tolist()
            assert src[0][:len(usable)].tobytes() == one.lattice_track_decode_src[[lo + j for j in usable]].tobytes()
    finally:
        pool.close()


def test_a_lexicon_lattice_pool_and_the_new_pool_at_once(scene):  # noqa: F811
    S, f, frames, read, table, plain, res = scene
    f.set_lexicon(read, fold_case=False)
    wants = dict(LWANTS, want_word_match=True, want_track_read=True)
    pools = [S.TrackPool(f, 256, lattice=True), S.TrackPool(f, 256, lattice=True), S.LatticeDecodePool(f, 256, keep=8), S.LatticeDecodePool(f, 300, keep=8)]
    try:
        alone, beside, decode = S.WordTracker(f, pools[0]), S.WordTracker(f, pools[1], pools[2]), S.WordTracker(f, decode_pool=pools[3])
        for lo in range(0, 8, 4):
            part = f.text_detect_list(frames[lo:lo + 4], GROUPED, **wants)
            ids = [t.update(part).tolist() for t in (alone, beside, decode)]
            assert ids[0] == ids[1] == ids[2] and alone._slot == beside._slot == decode._slot
        every = list(range(len(alone._parent)))
        assert len(every) > 0 and beside.read(every).tobytes() == alone.read(every).tobytes()          # the lexicon side: byte for byte
        assert all(a.tobytes() == b.tobytes() for a, b in zip(beside.read_decode(every), decode.read_decode(every)))
        assert [(i, r.tobytes(), c.tobytes()) for i, r, c in beside.closed_decodes] == [(i, r.tobytes(), c.tobytes()) for i, r, c in decode.closed_decodes]
        assert pools[1].info()["in_use"] == pools[2].info()["in_use"] == pools[0].info()["in_use"]
    finally:
        for p in pools:
            p.close()
        f.set_lexicon([])


def test_a_folded_result_is_refused_before_either_pool_is_touched(scene):  # noqa: F811
    S, f, frames, read, table, plain, res = scene
    f.set_lexicon(read)          # fold_case
    pools = [S.TrackPool(f, 64, lattice=True), S.LatticeDecodePool(f, 64, keep=4)]
    try:
        part = f.text_detect_list(frames[:2], GROUPED, want_word_match=True, want_track_read=True, **LWANTS)
        tracker = S.WordTracker(f, pools[0], pools[1])
        with pytest.raises(ValueError):
            tracker.update(part)
        assert pools[0].info()["in_use"] == 0 and pools[1].info()["in_use"] == 0 and tracker._slot == {}
    finally:
        for p in pools:
            p.close()
        f.set_lexicon([])
