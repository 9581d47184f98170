"""STR_ER_WANT_LINE_LINKS / str_er_link_feet on the GPU: the overlaps of the lines of adjacent frames, the links, the text tracks, the
edge feet and TextTracker against the numpy reference (line_links_ref.py, frame_lines_ref.py), bit for bit."""
import numpy as np
import pytest

import frame_lines_ref as FR
import line_links_ref as R
from test_frame_lines import FOOT, GROUPED, _cols, _ctx, _same, check as check_frame_lines, reference as frame_lines_reference

pytestmark = pytest.mark.gpu


def _feet(S, feet):
    """Reference footprints as the arguments of link_feet: LINE_FOOT_DTYPE records and the words back to back."""
    ft = np.zeros(len(feet), S.LINE_FOOT_DTYPE)
    for t, f in enumerate(feet):
        ft[t]["x"], ft[t]["y"], ft[t]["w"], ft[t]["h"], ft[t]["pixels"] = f.x, f.y, f.w, f.h, f.pixels
    return ft, np.concatenate([f.words() for f in feet] + [np.zeros(0, "<u4")])


def _tight(bits):
    """Random bits whose bounding box is the whole array."""
    bits = bits.copy()
    bits[0, 0] = bits[-1, -1] = True
    return bits


def _link_rows(got):
    return [(int(p["a"]), int(p["b"]), int(p["inter"]), int(p["link"])) for p in got]


# ---- str_er_link_feet on hand-made footprints ---------------------------------------------------------------------------------------------

W, H = 6000, 400


def _hand_made(rng):
    """Two sets of footprints on a 6000 x 400 frame, built as bit arrays.  Returns (A, B, named indices)."""
    A, B, at = [], [], {}
    full = lambda h, w: np.ones((h, w), bool)
    A.append(FR.Foot(3, 10, full(6, 290)))                              # a bar wider than 64 pixels ...
    at["wide"] = 0
    for k in range(64):                                                 # ... against 64 bars whose x origins take every residue modulo 64 to it
        B.append(FR.Foot(5 + k, 12 + (k % 3), _tight(rng.random((3, 70 + k % 5)) < 0.7)))
    at["huge"] = (len(A), len(B))                                       # a footprint wider than 4096 pixels, and one that crosses its far end
    A.append(FR.Foot(100, 100, _tight(rng.random((3, 4500)) < 0.5)))
    B.append(FR.Foot(4400, 99, _tight(rng.random((5, 400)) < 0.5)))
    same = _tight(rng.random((8, 50)) < 0.5)                            # two identical footprints: Jaccard 1
    at["same"] = (len(A), len(B))
    A.append(FR.Foot(500, 200, same)); B.append(FR.Foot(500, 200, same.copy()))
    ring = full(30, 50); ring[6:24, 6:44] = False                       # a ring and a bar in its hole: nested boxes, no common pixel
    at["nested"] = (len(A), len(B))
    A.append(FR.Foot(1000, 200, ring)); B.append(FR.Foot(1010, 210, full(10, 30)))
    at["exact"] = (len(A), len(B))                                      # 300 and 300 pixels, 200 common: 200 * 2 == 1 * 400
    A.append(FR.Foot(2000, 300, full(10, 30))); B.append(FR.Foot(2010, 300, full(10, 30)))
    below = full(10, 30); below[4, 5] = False                           # ... and with one of the common pixels missing
    at["below"] = (len(A), len(B))
    A.append(FR.Foot(2100, 300, full(10, 30))); B.append(FR.Foot(2110, 300, below))
    at["exact3"] = (len(A), len(B))                                     # at 1 / 3: 300 and 300, 150 common: 150 * 3 == 450
    A.append(FR.Foot(2200, 300, full(10, 30))); B.append(FR.Foot(2215, 300, full(10, 30)))
    at["shifted"] = (len(A), len(B))                                    # eight random blocks against themselves moved by 1 .. 8 pixels
    for i in range(8):
        blk = _tight(rng.random((12, 60)) < 0.8)
        A.append(FR.Foot(200 + 100 * i, 300, blk)); B.append(FR.Foot(201 + 100 * i + i, 300, blk.copy()))
    A.append(FR.Foot())                                                 # an empty footprint in a set
    at["grid"] = (len(A), len(B))                                       # 36 vertical bars x 36 horizontal bars: 1296 pairs of 6 pixels
    for i in range(36):
        A.append(FR.Foot(3000 + 8 * i, 150, full(216, 3)))
    for j in range(36):
        B.append(FR.Foot(3000, 150 + 6 * j, full(2, 288)))
    return A, B, at


def test_link_feet_hand_made(S, cascade_paths):
    A, B, at = _hand_made(np.random.default_rng(7))
    ref = R.set_links(A, B)
    by = {(a, b): (k, l) for a, b, k, l in ref}
    # the properties the sets were made for, on the reference alone
    assert A[at["wide"]].w > 64 and all((0, k) in by for k in range(64))
    assert {(B[k].x - A[0].x) % 64 for k in range(64)} == set(range(64))
    ha, hb = at["huge"]
    assert A[ha].w > 4096 and (ha, hb) in by and B[hb].x + B[hb].w > A[ha].x + 4096
    sa, sb = at["same"]
    assert by[(sa, sb)] == (A[sa].pixels, 1) and A[sa].pixels == B[sb].pixels
    na, nb = at["nested"]
    assert (na, nb) not in by and A[na].x < B[nb].x and B[nb].x + B[nb].w < A[na].x + A[na].w and A[na].y < B[nb].y
    ea, eb = at["exact"]
    k = by[(ea, eb)][0]
    assert k * 2 == A[ea].pixels + B[eb].pixels - k and by[(ea, eb)][1] == 1
    ba, bb = at["below"]
    k = by[(ba, bb)][0]
    assert by[(ba, bb)][1] == 0 and k * 2 < A[ba].pixels + B[bb].pixels - k and (k + 1) * 2 == A[ba].pixels + B[bb].pixels + 1 - (k + 1)
    n_lines = len(A) + len(B)
    assert len(ref) > max(1024, 4 * n_lines)                            # more than the first table: the overflow pass runs on a fresh context
    assert sum(l for *_, l in ref) >= 4 and sum(1 - l for *_, l in ref) > 100
    fa, wa = _feet(S, A)
    fb, wb = _feet(S, B)
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=1)
    got = f.link_feet(W, H, fa, wa, fb, wb)
    assert _link_rows(got) == ref
    assert _link_rows(f.link_feet(W, H, fa, wa, fb, wb)) == ref         # (again: the table now holds them all)
    # the other way round: b against a
    assert _link_rows(f.link_feet(W, H, fb, wb, fa, wa)) == R.set_links(B, A)
    # other thresholds: exactly at 1 / 3, and 1 / 1 (identical footprints only)
    f.set_line_link(1, 3)
    ref3 = R.set_links(A, B, 1, 3)
    xa, xb = at["exact3"]
    k = {(a, b): k for a, b, k, _ in ref3}[(xa, xb)]
    assert k * 3 == A[xa].pixels + B[xb].pixels - k and (xa, xb, k, 1) in ref3 and (xa, xb, k, 0) in ref
    assert _link_rows(f.link_feet(W, H, fa, wa, fb, wb)) == ref3
    f.set_line_link(1, 1)
    ref1 = R.set_links(A, B, 1, 1)
    assert [r for r in ref1 if r[3]] == [(sa, sb, A[sa].pixels, 1)]
    assert _link_rows(f.link_feet(W, H, fa, wa, fb, wb)) == ref1
    for bad in ((0, 1), (2, 1), (1, 65536)):
        with pytest.raises(S.StrErError):
            f.set_line_link(*bad)
    assert _link_rows(f.link_feet(W, H, fa, wa, fb, wb)) == ref1        # (a refused threshold changes nothing)
    f.set_line_link(1, 2)
    # an empty set on either side, and sets of empty footprints
    none_f, none_w = _feet(S, [])
    assert len(f.link_feet(W, H, none_f, none_w, fb, wb)) == 0 and len(f.link_feet(W, H, fa, wa, none_f, none_w)) == 0
    assert len(f.link_feet(W, H, none_f, none_w, none_f, none_w)) == 0
    ef, ew = _feet(S, [FR.Foot(), FR.Foot()])
    assert len(f.link_feet(W, H, ef, ew, fb, wb)) == 0 and len(f.link_feet(W, H, fa, wa, ef, ew)) == 0
    # malformed input is refused, the context stays usable
    one, one_w = _feet(S, [FR.Foot(10, 10, np.ones((4, 40), bool))])
    for change in ("leaves", "pixels", "tail", "size"):
        ft, wd, fw, fh = one.copy(), one_w.copy(), W, H
        if change == "leaves":
            ft[0]["x"] = W - 39
        elif change == "pixels":
            ft[0]["pixels"] += 1
        elif change == "tail":
            wd[1] |= np.uint32(1 << 8)
        else:
            fw = 65536
        with pytest.raises(S.StrErError) as e:
            f.link_feet(fw, fh, ft, wd, fb, wb)
        assert e.value.code == -1, change
    assert _link_rows(f.link_feet(W, H, fa, wa, fb, wb)) == ref
    f.close()


def test_link_feet_feet_geom_and_feet_words_in_turn(S, cascade_paths):
    """The three calls on a caller's footprints share the context's line table and footprint words: one after the other on one context,
    each with another number of footprints, twice, each result against its reference with ==."""
    import line_geom_ref as G
    import line_words_ref as WD
    rng = np.random.default_rng(11)
    bar = np.ones((3, 70), bool)
    bar[:, 20:24] = False                                               # two glyph runs, 70 columns: two device words a row
    items = [(5, 10, bar), (30, 11, _tight(rng.random((2, 65)) < 0.6)), (40, 12, _tight(rng.random((3, 33)) < 0.6))]
    feet = [FR.Foot(x, y, b) for x, y, b in items]
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=1)
    ref_links = R.set_links(feet[:2], feet[2:])
    assert len(ref_links) == 2
    for _ in range(2):
        assert _link_rows(f.link_feet(200, 100, *_feet(S, feet[:2]), *_feet(S, feet[2:]))) == ref_links          # three lines
        geoms, points = f.feet_geom(200, 100, *_feet(S, [feet[2], feet[0]]))                                      # two
        assert len(geoms) == 2 and len(points) == sum(len(G.geom(b, x, y)[3]) for x, y, b in (items[2], items[0]))
        for g, (x, y, b) in zip(geoms, (items[2], items[0])):
            assert G.same(g, points, G.geom(b, x, y)) is None
        got = WD.as_lists(*f.feet_words(200, 100, *_feet(S, [feet[1]])))                                          # one
        assert list(got) == list(WD.tables([items[1]]))
    f.close()


# ---- the fused call ---------------------------------------------------------------------------------------------------------------------

MOTION = (2, 1)          # pixels per frame, x and y
SEGMENTS = ((640, 480, 401, 6), (640, 480, 402, 6), (448, 336, 402, 4))       # (width, height, canvas seed, frames): a cut, then a change of size


def make_video(S, motion=MOTION, segments=SEGMENTS):
    """A window moving over an S-text canvas, `motion` pixels a frame; a scene cut to another canvas; then a smaller window."""
    frames, seg_of = [], []
    canvases = {}
    for s, (w, h, seed, n) in enumerate(segments):
        if seed not in canvases:
            canvases[seed] = S.synth.stext_bgr(S.synth.frame_seed(seed), 720, 540)
        for i in range(n):
            x, y = 8 + motion[0] * i, 6 + motion[1] * i
            frames.append(np.ascontiguousarray(canvases[seed][y:y + h, x:x + w]))
            seg_of.append(s)
    return frames, seg_of


def reference(res, sizes, num=1, den=2):
    """The frame lines, links and tracks of a result that carries its masks (want_masks=True), by the references."""
    fl = frame_lines_reference(res, sizes)
    feet, pairs, dup = fl[0], fl[1], fl[2]
    frames = [int(t["frame"]) for t in res.texts]
    links = R.adjacent_links(feet, frames, sizes)
    pixels = [f.pixels for f in feet]
    link, track, tracks, members = R.text_tracks(pixels, frames, [(a, b, d) for (a, b, _), d in zip(pairs, dup)], links, num, den)
    return fl, feet, frames, links, link, track, tracks, members


def check(S, res, ref, n_frames):
    fl, feet, frames, links, link, track, tracks, members = ref
    check_frame_lines(res, fl)
    assert [(int(p["a"]), int(p["b"]), int(p["inter"])) for p in res.line_links] == links
    assert [int(p["link"]) for p in res.line_links] == link
    assert [int(v) for v in res.line_tracks] == track
    assert [{k: int(g[k]) for k in g.dtype.names} for g in res.text_tracks] == tracks
    assert [int(m) for m in res.text_track_members] == members
    for which, f in ((0, 0), (1, n_frames - 1)):
        e = res.edge_feet(which)
        mine = [t for t in range(len(feet)) if frames[t] == f]
        assert [int(t) for t in e.lines] == mine
        ft, wd = _feet(S, [feet[t] for t in mine])
        assert e.feet[["x", "y", "w", "h", "pixels"]].tolist() == ft[["x", "y", "w", "h", "pixels"]].tolist()
        assert e.bits.tobytes() == wd.tobytes()


def video_properties(ref, seg_of, say=print):
    """What the video must show for the test to mean anything, on the reference alone: (a track over a whole segment, an overlap that is
    no link, lines on both sides of the change of size and no overlap recorded across it)."""
    fl, feet, frames, links, link, track, tracks, members = ref
    seg_frames = {s: [f for f, q in enumerate(seg_of) if q == s] for s in set(seg_of)}
    spans = [s for s, fs in seg_frames.items() if any(g["first_frame"] <= fs[0] and g["last_frame"] >= fs[-1] for g in tracks)]
    change = [f for f in range(1, len(seg_of)) if seg_of[f] != seg_of[f - 1]][-1]           # the first frame of the other size
    across = [(a, b) for a, b, _ in links if frames[a] == change - 1 and frames[b] == change]
    both = any(f == change - 1 for f in frames) and any(f == change for f in frames)
    say("lines", len(feet), "overlaps", len(links), "links", sum(link), "overlaps that are no link", len(link) - sum(link), "tracks", len(tracks),
        "segments spanned by a track", spans, "longest track", max([g["last_frame"] - g["first_frame"] + 1 for g in tracks] + [0]),
        "lines on both sides of the size change", both, "overlaps across it", len(across))
    return bool(spans), len(link) - sum(link) > 0, both and not across


def test_fused_video_list_stream_and_tracker(S, cascade_paths):
    """A 16-frame video (make_video) through one list call on a 3-level pyramid context: every table against the reference built from
    the call's own masks and lines.  The video must give the reference something to decide -- asserted, not skipped."""
    prm = S.Params(max_width=640, max_height=480, max_frames=16, n_pyr_levels=3)
    f = S.ERFilter(params=prm)
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    frames, seg_of = make_video(S)
    sizes = [(fr.shape[1], fr.shape[0]) for fr in frames]
    res = f.text_detect_list(frames, GROUPED, want_masks=True, want_frame_lines=True, want_line_links=True)
    ref = reference(res, sizes)
    spans, unlinked, size_change = video_properties(ref, seg_of)
    assert spans, "no track spans a whole segment: change the motion"
    assert unlinked, "every overlap is a link: change the motion"
    assert size_change, "the change of size shows nothing"
    check(S, res, ref, len(frames))
    # the flag changes nothing else: the frame-line tables and every other table of the call are byte-identical without it
    plain = f.text_detect_list(frames, GROUPED, want_masks=True, want_frame_lines=True)
    _same(plain, res)
    for k in ("line_feet", "line_pairs", "frame_lines", "frame_line_members"):
        assert getattr(plain, k).tobytes() == getattr(res, k).tobytes(), k
    with pytest.raises(ValueError):
        plain.line_links
    with pytest.raises(ValueError):
        plain.edge_feet(0)
    # without the masks in the result (the stage makes the members' masks itself)
    lean = f.text_detect_list(frames, GROUPED, want_frame_lines=True, want_line_links=True)
    for k in ("line_links", "line_tracks", "text_tracks", "text_track_members"):
        assert getattr(lean, k).tobytes() == getattr(res, k).tobytes(), k
    # the equal-size part as one batch call (str_er_detect_bgr): the tables of the list call's first 12 frames
    n12 = sum(s < 2 for s in seg_of)
    batch = f.text_detect(np.stack(frames[:n12]), GROUPED, want_masks=True, want_frame_lines=True, want_line_links=True)
    check(S, batch, reference(batch, sizes[:n12]), n12)
    # the flag without WANT_FRAME_LINES is refused, and the context stays usable
    with pytest.raises(S.StrErError) as e:
        f.text_detect_list(frames, GROUPED, want_line_links=True)
    assert e.value.code == -1 and "STR_ER_WANT_LINE_LINKS" in str(e.value)
    # the same video through a FrameStream in four submissions, TextTracker joining them: the ids are the tracks of the one call
    st = S.FrameStream(prm, depth=2)
    st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
    tracker = S.TextTracker(f)
    flags = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_LINKS
    ids, feet_bytes = [], b""
    for lo, hi in ((0, 5), (5, 9), (9, 12), (12, 16)):
        slot, buf = st.acquire()
        layout, off = [], 0
        for fr in frames[lo:hi]:
            h, w = fr.shape[:2]
            buf[off:off + 3 * w * h] = fr.reshape(-1)
            layout.append((off, w, h, 3 * w))
            off += (3 * w * h + 255) // 256 * 256
        st.submit_list(slot, layout, flags)
        _, part = st.next()
        assert int(part.texts["frame"].max()) < hi - lo if len(part.texts) else True
        ids.append(tracker.update(part))
        feet_bytes += _cols(part.line_feet, FOOT)
    assert feet_bytes == _cols(res.line_feet, FOOT)        # (the same lines, in the same order)
    ids = tracker.resolve(np.concatenate(ids))
    track = res.line_tracks
    assert len(ids) == len(track)
    fwd, back = {}, {}
    for i, t in zip(ids.tolist(), track.tolist()):
        assert fwd.setdefault(i, t) == t and back.setdefault(t, i) == i, (i, t)
    assert len(fwd) == len(res.text_tracks)
    st.close(); f.close()


def test_one_frame_and_no_lines(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=2, n_pyr_levels=2)
    frame = S.synth.stext_bgr(S.synth.frame_seed(2), 640, 480)
    one = f.text_detect(frame, GROUPED, want_masks=True, want_frame_lines=True, want_line_links=True)
    assert len(one.texts) > 0 and len(one.line_links) == 0
    check(S, one, reference(one, [(640, 480)]), 1)
    assert one.edge_feet(0).bits.tobytes() == one.edge_feet(1).bits.tobytes()
    # the same frame twice: every line is linked to itself in the next frame
    two = f.text_detect(np.stack([frame, frame]), GROUPED, want_masks=True, want_frame_lines=True, want_line_links=True)
    ref = reference(two, [(640, 480)] * 2)
    check(S, two, ref, 2)
    n = len(one.texts)
    assert all((t, n + t, int(one.line_feet[t]["pixels"])) in ref[3] for t in range(n)) and all(g["last_frame"] == 1 for g in ref[6])
    blank = f.text_detect(np.full((2, 120, 160, 3), 128, np.uint8), GROUPED, want_frame_lines=True, want_line_links=True)
    assert len(blank.texts) == 0 and len(blank.line_links) == 0 and len(blank.line_tracks) == 0 and len(blank.text_tracks) == 0
    assert len(blank.edge_feet(0).lines) == 0 and (blank.edge_feet(1).width, blank.edge_feet(1).height) == (160, 120)
    f.close()
