"""STR_ER_WANT_LINE_WORDS / str_er_feet_words on the GPU: the glyph runs and words of every footprint and of every line against the
reference (line_words_ref.py, frame_lines_ref.py), every field with ==."""
import ctypes as C

import numpy as np
import pytest

import frame_lines_ref as FR
import line_words_ref as R
from test_frame_lines import GROUPED, _crops, _ctx, _same, reference as frame_lines_reference

pytestmark = pytest.mark.gpu
W, H = 5000, 20000                      # the frame of the hand-made footprints: room for 4100 columns and 16385 rows
TABLES = ("line_words", "line_runs", "words")


def _feet(S, items):
    """(x0, y0, bits) footprints as the arguments of feet_words: LINE_FOOT_DTYPE records and the words back to back."""
    feet = [FR.Foot(x, y, b) if b.size else FR.Foot() for x, y, b in items]
    ft = np.zeros(len(feet), S.LINE_FOOT_DTYPE)
    for t, f in enumerate(feet):
        ft[t]["x"], ft[t]["y"], ft[t]["w"], ft[t]["h"], ft[t]["pixels"] = f.x, f.y, f.w, f.h, f.pixels
    return ft, np.concatenate([f.words() for f in feet] + [np.zeros(0, "<u4")])


def _run(S, f, items, num=1, den=3):
    """feet_words on the footprints, held against the reference; returns (the reference's tables, the three arrays)."""
    got = f.feet_words(W, H, *_feet(S, items))
    ref = R.tables(items, num, den)
    lists = R.as_lists(*got)
    for name, a, b in zip(TABLES, lists, ref):
        assert a == b, name
    return ref, got


def _cols(w, h, cols, x=7, y=11):
    """A footprint of width w and height h with the given columns full."""
    b = np.zeros((h, w), bool)
    b[:, list(cols)] = True
    return x, y, b


EMPTY = (0, 0, np.zeros((0, 0), bool))


@pytest.fixture(scope="module")
def ctx(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=1)
    yield f
    f.close()


# ---- str_er_feet_words on hand-made footprints ---------------------------------------------------------------------------------------------

def test_one_pixel_and_several_rows(S, ctx):
    ref, got = _run(S, ctx, [(0, 0, np.ones((1, 1), bool))])
    assert ref == ([(0, 1, 0, 1, 1, 0)], [(0, 1, 0, 1, 1, 0)], [(0, 0, 1, 0, 0, 1, 1, 1)])
    ref, _ = _run(S, ctx, [(W - 1, H - 1, np.ones((1, 1), bool))])
    assert ref[1] == [(W - 1, W, H - 1, H, 1, 0)]
    b = np.zeros((5, 12), bool)
    b[0, 0:3] = b[2, 1:4] = b[4, 8:12] = b[1, 9] = True               # colmax 2 (column 9): the gap of 4 breaks at 1 / 3
    ref, _ = _run(S, ctx, [(3, 4, b)])
    assert ref[0] == [(0, 2, 0, 2, 2, 0)] and ref[1] == [(3, 7, 4, 7, 6, 0), (11, 15, 5, 9, 5, 1)]
    assert ref[2] == [(0, 0, 1, 3, 4, 4, 3, 6), (0, 1, 1, 11, 5, 4, 4, 5)]


def _edge_cases(w):
    """The footprints of width w (h = 3) around the 64-column words of the device: every one with its first and last column set."""
    out = {}
    ends = {0, w - 1}
    if w >= 65:
        out["ends_at_63"] = ends | set(range(58, 64))
        out["bits_0_and_63"] = ends | {63}
    if w >= 67:
        out["starts_at_64"] = ends | set(range(64, min(w - 2, 70)))
        out["straddles"] = ends | set(range(61, min(w - 2, 67)))
    if w >= 129:
        out["gap_is_word_1"] = set(range(0, 64)) | {128}
        out["single_columns"] = ends | {63, 65, 126}
    out["full"] = set(range(w))
    out["ends_only"] = ends
    out["alternate"] = set(range(0, w, 2)) | ends
    return out


def test_widths_around_the_device_words(S, ctx):
    items, names = [], []
    for w in (31, 32, 33, 63, 64, 65, 127, 128, 129):
        for name, cols in _edge_cases(w).items():
            x, y, b = _cols(w, 3, cols, x=5 + w % 7)
            b[1, list(cols)[::2]] = False                      # (not every column the same count)
            items.append((x, y, b))
            names.append((w, name))
    ref, got = _run(S, ctx, items)
    by = {n: ref[1][ref[0][i][2]:ref[0][i][2] + ref[0][i][3]] for i, n in enumerate(names)}
    x129 = 5 + 129 % 7
    assert [r[:2] for r in by[(129, "ends_at_63")]] == [(x129, x129 + 1), (x129 + 58, x129 + 64), (x129 + 128, x129 + 129)]
    assert [r[:2] for r in by[(129, "starts_at_64")]] == [(x129, x129 + 1), (x129 + 64, x129 + 70), (x129 + 128, x129 + 129)]
    assert [r[:2] for r in by[(129, "straddles")]] == [(x129, x129 + 1), (x129 + 61, x129 + 67), (x129 + 128, x129 + 129)]
    assert [r[:2] for r in by[(129, "gap_is_word_1")]] == [(x129, x129 + 64), (x129 + 128, x129 + 129)]
    assert [r[:2] for r in by[(129, "bits_0_and_63")]] == [(x129, x129 + 1), (x129 + 63, x129 + 64), (x129 + 128, x129 + 129)]
    assert len(by[(129, "single_columns")]) == 5 and len(by[(128, "full")]) == 1 and len(by[(127, "straddles")]) == 3
    # each alone as well (another slot and another grid)
    for item in items[::5]:
        _run(S, ctx, [item])


def test_alternating_columns_fill_the_reserved_slots(S, ctx):
    ref, _ = _run(S, ctx, [_cols(129, 2, range(0, 129, 2)), _cols(129, 2, range(0, 129, 2), x=300)])
    assert ref[0][0][3] == 65 == (129 + 1) // 2 and ref[0][1][2:4] == (65, 65)
    assert len(ref[2]) == 130                                  # colmax 2: every gap of 1 breaks at 1 / 3 (3 >= 2)


def test_more_than_64_device_words(S, ctx):
    sparse = _cols(4100, 2, [0, 1, 2, 700, 701, 2047, 2048, 3000, 4030] + list(range(4031, 4100)))
    long_run = _cols(4100, 2, [0] + list(range(4030, 4100)))
    dense = _cols(4100, 2, range(0, 4100, 2), x=1)                        # 2050 runs: past the runs the kernel combines in LDS
    ref, _ = _run(S, ctx, [sparse, long_run, dense])
    assert ref[1][ref[0][1][2] + 1][:2] == (7 + 4030, 7 + 4100) and ref[0][2][3] == 2050 > 1024
    assert ref[0][0][3] == 5
    _run(S, ctx, [dense])


def test_carry_planes_and_the_capacity(S, ctx):
    items = []
    for n in (1023, 1024, 1025):
        b = np.zeros((n, 2), bool)
        b[:, 0] = True
        b[n // 2, 1] = True
        items.append((9, 3, b))
    items.append((4, 0, np.ones((16384, 1), bool)))
    ref, _ = _run(S, ctx, items)
    assert [lw[4] for lw in ref[0]] == [1023, 1024, 1025, 16384]
    assert ref[1][-1] == (4, 5, 0, 16384, 16384, 3) and ref[1][0] == (9, 11, 3, 1026, 1024, 0)
    with pytest.raises(S.StrErError) as e:
        ctx.feet_words(W, H, *_feet(S, [(4, 0, np.ones((16385, 1), bool))]))
    assert e.value.code == -7
    with pytest.raises(S.StrErError) as e:
        ctx.feet_words(20000, 100, *_feet(S, [(0, 3, np.ones((1, 16385), bool))]))
    assert e.value.code == -7
    got = ctx.feet_words(20000, 100, *_feet(S, [(0, 3, np.ones((1, 16384), bool))]))
    assert R.as_lists(*got) == R.tables([(0, 3, np.ones((1, 16384), bool))])
    _run(S, ctx, items[:1])                                               # the context is usable afterwards


def test_row_extents(S, ctx):
    b = np.zeros((20, 30), bool)
    b[0, 0] = b[19, 29] = True                                            # the box
    b[5:8, 10:14] = True
    b[6, 12] = False
    two = np.zeros((20, 40), bool)
    two[2:9, 0:5] = True
    two[11:20, 6:12] = True                                               # a gap of 1: one word at 1 / 3 (colmax 9)
    two[0, 39] = True
    ref, _ = _run(S, ctx, [(50, 100, b), (60, 200, two)])
    assert ref[1][1] == (60, 64, 105, 108, 11, 1)
    assert ref[1][3:5] == [(60, 65, 202, 209, 35, 3), (66, 72, 211, 220, 54, 3)] and ref[2][3] == (1, 3, 2, 60, 202, 12, 18, 89)


def _random_feet(rng, n):
    items = []
    for t in range(n):
        if t % 9 == 4:
            items.append(EMPTY)
            continue
        w = int(rng.choice([1, 2, 5, 31, 64, 65, 100, 130, 257, 600]))
        h = int(rng.choice([1, 2, 3, 8, 17, 40, 70]))
        b = rng.random((h, w)) < rng.choice([0.02, 0.2, 0.6])
        b &= (rng.random(w) < rng.choice([0.3, 0.8, 1.0]))[None, :]        # whole columns out: gaps of any width
        if not b.any():
            b[h // 2, w // 2] = True
        rows, cols = np.nonzero(b.any(axis=1))[0], np.nonzero(b.any(axis=0))[0]
        b = b[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1].copy()
        items.append((int(rng.integers(0, W - 600)), int(rng.integers(0, H - 70)), b))
    return items


def test_many_footprints_growth_repeat_and_errors(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=1)
    rng = np.random.default_rng(8)
    items = _random_feet(rng, 300)
    assert sum(1 for it in items if it is EMPTY) > 30 and max(b.shape[1] for _, _, b in items) > 256
    small = items[:5]
    ref_small, got_small = _run(S, f, small)
    ref, got = _run(S, f, items)
    assert ref[0][4] == (ref[0][3][0] + ref[0][3][1], 0, ref[0][3][2] + ref[0][3][3], 0, 0, 0)          # an empty footprint between others
    assert max(lw[1] for lw in ref[0]) > 3 and any(lw[3] > lw[1] > 0 for lw in ref[0])                  # words of several runs, lines of several words
    _, again_small = _run(S, f, small)                                     # small, large, small: the buffers grew once and are reused
    _, again = _run(S, f, items)
    for a, b in zip(got + got_small, again + again_small):
        assert a.tobytes() == b.tobytes()                                  # byte-identical when repeated
    # the gap of the context: every gap, no gap, and what it refuses
    f.set_word_gap(1, 65535)
    ref_all, _ = _run(S, f, items, 1, 65535)
    assert len(ref_all[2]) == len(ref_all[1])
    f.set_word_gap(65535, 1)
    ref_none, _ = _run(S, f, items, 65535, 1)
    assert len(ref_none[2]) == sum(1 for lw in ref_none[0] if lw[3]) < len(ref[2]) < len(ref_all[2])
    for num, den in ((0, 3), (65536, 3), (1, 0), (1, 65536), (-1, 3)):
        with pytest.raises(S.StrErError) as e:
            f.set_word_gap(num, den)
        assert e.value.code == -1
    _run(S, f, small, 65535, 1)                                            # the context unchanged by the refusals
    f.set_word_gap()
    _run(S, f, small)
    # nothing at all, only empty footprints, and the counting call
    lw, runs, words = f.feet_words(W, H, *_feet(S, []))
    assert len(lw) == 0 and len(runs) == 0 and len(words) == 0
    lw, runs, words = f.feet_words(W, H, *_feet(S, [EMPTY, EMPTY]))
    assert R.as_lists(lw, runs, words) == ([(0, 0, 0, 0, 0, 0)] * 2, [], [])
    ft, wd = _feet(S, small)
    nr, nw = C.c_int32(), C.c_int32()
    out = np.zeros(len(ft), S.LINE_WORDS_DTYPE)
    assert f.L.str_er_feet_words(f.h, W, H, ft.ctypes.data, wd.ctypes.data, len(ft), out.ctypes.data, None, 0, C.byref(nr), None, 0, C.byref(nw)) == 0
    assert (nr.value, nw.value) == (len(ref_small[1]), len(ref_small[2])) and out.tobytes() == got_small[0].tobytes()
    few = np.zeros(1, S.LINE_RUN_DTYPE)
    many = np.zeros(len(ref_small[2]), S.LINE_WORD_DTYPE)
    assert f.L.str_er_feet_words(f.h, W, H, ft.ctypes.data, wd.ctypes.data, len(ft), out.ctypes.data, few.ctypes.data, 1, C.byref(nr), many.ctypes.data,
                                 len(many), C.byref(nw)) == -7
    assert (nr.value, nw.value) == (len(ref_small[1]), len(ref_small[2]))
    # malformed input is refused as str_er_link_feet refuses it, the context stays usable
    one, one_w = _feet(S, [(10, 10, np.ones((4, 40), bool))])
    for change in ("leaves", "pixels", "tail", "size", "box"):
        a, b, fw = one.copy(), one_w.copy(), W
        if change == "leaves":
            a[0]["x"] = W - 39
        elif change == "pixels":
            a[0]["pixels"] += 1
        elif change == "tail":
            b[1] |= np.uint32(1 << 8)
        elif change == "box":
            a[0]["h"] = 0
            b = b[:0]
        else:
            fw = 65536
        with pytest.raises(S.StrErError) as e:
            f.feet_words(fw, H, a, b)
        assert e.value.code == -1, change
    _, last = _run(S, f, items)
    for a, b in zip(got, last):
        assert a.tobytes() == b.tobytes()
    f.close()


# ---- the fused call ---------------------------------------------------------------------------------------------------------------------

def check(res, sizes, num=1, den=3):
    """The three tables of a result that carries its masks (want_masks=True) and frame lines against the references."""
    feet = frame_lines_reference(res, sizes)[0]
    ref = R.tables([(f.x, f.y, f.bits) for f in feet], num, den)
    got = R.as_lists(res.line_words, res.line_runs, res.words)
    for name, a, b in zip(TABLES, got, ref):
        assert a == b, name
    assert len(res.line_words) == len(res.texts)
    for t in range(len(res.texts)):
        lw = ref[0][t]
        assert [tuple(int(v) for v in w) for w in res.words_of_line(t).tolist()] == ref[2][lw[0]:lw[0] + lw[1]]
        assert [tuple(int(v) for v in r) for r in res.runs_of_line(t).tolist()] == ref[1][lw[2]:lw[2] + lw[3]]
    for i, g in enumerate(res.frame_lines):
        assert res.frame_line_words(i).tobytes() == res.words_of_line(int(g["rep"])).tobytes()
    return ref


def test_fused_one_frame_and_a_list(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=2, n_pyr_levels=4)
    sy = S.synth
    frame = sy.stext_bgr(sy.frame_seed(2), 640, 480)                 # the frame of test_frame_lines.py::test_threshold
    frames = [frame, sy.stext_bgr(sy.frame_seed(971), 333, 211)]
    counts = {}
    for num, den in ((1, 3), (1, 65535), (65535, 1)):
        f.set_word_gap(num, den)
        res = f.text_detect(frame, GROUPED, want_masks=True, want_frame_lines=True, want_line_words=True)
        ref = check(res, [(640, 480)], num, den)
        assert len(ref[0]) > 0 and any(lw[3] >= 2 for lw in ref[0])             # some line has at least 2 runs
        lst = f.text_detect_list(frames, GROUPED, want_masks=True, want_frame_lines=True, want_line_words=True)
        assert {int(t["frame"]) for t in lst.texts} == {0, 1}
        counts[(num, den)] = (len(check(lst, [(640, 480), (333, 211)], num, den)[2]), len(lst.line_runs), sum(1 for lw in lst.line_words if lw["n_runs"]))
        # without the masks in the result (the stage makes the members' masks itself), and beside the links and the geometry
        for kw in ({}, {"want_line_links": True, "want_line_geom": True}):
            lean = f.text_detect_list(frames, GROUPED, want_frame_lines=True, want_line_words=True, **kw)
            for k in TABLES:
                assert getattr(lean, k).tobytes() == getattr(lst, k).tobytes(), (kw, k)
    assert counts[(1, 65535)][0] == counts[(1, 65535)][1] and counts[(65535, 1)][0] == counts[(65535, 1)][2]      # every gap a break; no gap a break
    assert counts[(65535, 1)][0] < counts[(1, 65535)][0]                                                            # both outcomes of the rule occur
    f.set_word_gap()
    # a grouped call without lines: empty tables, not an error
    blank = f.text_detect(np.full((120, 160, 3), 128, np.uint8), GROUPED, want_frame_lines=True, want_line_words=True)
    assert len(blank.texts) == 0 and len(blank.line_words) == 0 and len(blank.line_runs) == 0 and len(blank.words) == 0
    f.close()


def test_nv12_list_and_the_stream(S, cascade_paths):
    prm = S.Params(max_width=640, max_height=480, max_frames=8, n_pyr_levels=3)
    f = S.ERFilter(params=prm)
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    sy = S.synth
    flags = GROUPED | S.WANT_FRAME_LINES
    frames = _crops()[:2] + [sy.stext_bgr(sy.frame_seed(971), 333, 211), sy.stext_bgr(sy.frame_seed(972), 517, 301)]
    lst = f.text_detect_list(frames, GROUPED, want_frame_lines=True, want_line_words=True)
    assert len(lst.line_runs) > 0 and len(lst.words) > 0
    st = S.FrameStream(prm, depth=2)
    st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
    for want in (True, True, False):
        if want:
            st.submit_copy_list(frames, flags, want_line_words=True)
        else:
            st.submit_copy_list(frames, flags)
        _, a = st.next()
        if not want:
            with pytest.raises(ValueError):
                a.line_words
            continue
        for k in TABLES:
            assert getattr(a, k).tobytes() == getattr(lst, k).tobytes(), k
    st.close()
    nvf = [sy.stext_bgr(sy.frame_seed(976), 640, 480), sy.stext_bgr(sy.frame_seed(977), 322, 244)]
    nv = [sy.nv12_from_bgr(b) for b in nvf]
    nres = f.text_detect_nv12_list(nv, flags | S.WANT_LINE_WORDS | S.WANT_MASKS)
    assert len(nres.texts) > 0
    check(nres, [(b.shape[1], b.shape[0]) for b in nvf])
    one = f.text_detect_nv12(nv[0], 640, 480, flags | S.WANT_LINE_WORDS)
    n0 = len(one.texts)
    assert n0 > 0 and nres.line_words[:n0].tobytes() == one.line_words.tobytes() and nres.line_runs[:len(one.line_runs)].tobytes() == one.line_runs.tobytes()
    f.close()


def test_line_words_change_nothing_else(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=4, n_pyr_levels=2)
    sy = S.synth
    frames = [sy.stext_bgr(sy.frame_seed(2), 640, 480), _crops()[1], sy.snoise_bgr(sy.frame_seed(980), 200, 100)]
    every = (S.WANT_NODES | S.WANT_MASKS | S.WANT_SHAPES | S.WANT_STROKES | S.WANT_LINE_CROPS | S.WANT_LINE_GLYPHS | S.WANT_TEXT_MAP |
             S.WANT_LINE_MAP | S.WANT_LINE_LINKS | S.WANT_LINE_GEOM)
    got = []
    for extra in (0, S.WANT_MASKS, every):
        plain = f.text_detect_list(frames, GROUPED | S.WANT_FRAME_LINES | extra)
        with pytest.raises(ValueError):
            plain.line_words
        r = f.text_detect_list(frames, GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS | extra)
        _same(plain, r)
        for k in ("line_feet", "line_pairs", "frame_lines", "frame_line_members"):
            assert getattr(plain, k).tobytes() == getattr(r, k).tobytes(), k
        if extra & S.WANT_LINE_LINKS:
            for k in ("line_links", "line_tracks", "text_tracks", "text_track_members", "line_geoms", "frame_line_geoms", "geom_points"):
                assert getattr(plain, k).tobytes() == getattr(r, k).tobytes(), k
        got.append(r)
    for r in got[1:]:
        for k in TABLES:
            assert getattr(r, k).tobytes() == getattr(got[0], k).tobytes(), k
    assert len(got[0].texts) > 0 and len(got[0].words) > 0
    f.close()


def test_errors(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=320, max_height=240, max_frames=1)
    frame = S.synth.stext_bgr(S.synth.frame_seed(981), 320, 240)
    good = f.text_detect(frame, GROUPED, want_frame_lines=True, want_line_words=True)

    def usable():
        again = f.text_detect(frame, GROUPED, want_frame_lines=True, want_line_words=True)
        for k in TABLES:
            assert getattr(again, k).tobytes() == getattr(good, k).tobytes()

    with pytest.raises(S.StrErError) as e:                           # without STR_ER_WANT_FRAME_LINES
        f.text_detect(frame, GROUPED, want_line_words=True)
    assert e.value.code == -1 and "STR_ER_WANT_LINE_WORDS" in str(e.value)
    usable()
    planes = f.compute_channels(frame)                               # the per-plane calls
    with pytest.raises(S.StrErError) as e:
        f.detect_planes(planes[:1], S.STAGE_ALL | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS)
    assert e.value.code == -1 and "STR_ER_WANT_LINE_WORDS" in str(e.value)
    usable()
    with pytest.raises(S.StrErError) as e:
        f.detect_planes_list([planes[0], planes[1][:100, :90]], S.STAGE_ALL | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS)
    assert e.value.code == -1 and "STR_ER_WANT_LINE_WORDS" in str(e.value)
    usable()
    blob = (C.c_char * 16)()                                         # the strip path
    blobs = (C.c_void_p * 1)(C.cast(blob, C.c_void_p))
    sizes = (C.c_int64 * 1)(16)
    rh = C.c_void_p()
    rc = f.L.str_er_strip_merge(f.h, frame.ctypes.data, 320, 240, 960, 0, C.cast(blobs, C.c_void_p), C.cast(sizes, C.c_void_p), 1,
                                S.STAGE_ALL | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS, C.byref(rh))
    assert rc == -1 and b"STR_ER_WANT_LINE_WORDS" in f.L.str_er_last_error(f.h)
    usable()
    f.close()
