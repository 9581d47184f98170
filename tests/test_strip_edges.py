"""The strip path on hand-made planes at the cuts' own edges (api_strips.cpp: str_er_strip_extract[_dev] -- the cut, the phantom tile rows, the blanked
seam row, k_strip_border_ids; str_er_strip_merge[_ex] -- k_rebase_records, k_check_forest, k_connect_cut, the lo / hi walk over strips without rows).

Every plane of tests/strip_planes.py (tests/test_strip_planes.py proves with the cut census that each is what it is named for) goes, as a gray BGR frame
with channel_mask 0x09 (the plane and its complement), through one worker context per strip and an owner context:

  main check      merged `cands`, `info` and every plane's `nodes` are the bytes `text_detect` gives for the same frame, and every plane passes
                  check_plane_against_oracle -- at MIN_AREA 120 and 1, for every strip count of the case (1, 2, a strip a tile row, one strip more than
                  tile rows, empty strips between strips with rows), widths 1 .. 257, heights 33 .. 97
  the blob alone  header (`row0`, `rows`) and every StripPlane (`has_top`, `has_bot`) against strip_planes.cut_rows; every entry of a top / bot row is NONE
                  iff its pixel is a wall, else below n_nodes and names a record whose level byte is the pixel's quantised level
  thresh steps    rings, serpent, levels_across and wall_cut at EVERY step the sentinel rule accepts (2, 4, 8, 10, 13, 16, 20, 22, 24, 26, 29, 32: see
                  test_strip_planes.test_sentinel_rule_in_float32); 1, 3 and 6 are refused with STR_ER_EINVAL from a strip with rows above it only
  configurations  the planes of one size under every entry of test_tree_edges.CONFIGS on workers and owner: the same node tables everywhere
  entry points    strip_extract_dev + strip_merge_ex(device_blobs=True); plane_select; dist.detect_frame_strips over an in-process group of 4 on 40 rows
  stages          strip_merge with STAGE_TRACK | STAGE_GROUP against text_detect with the same stages
  one grid round  two strips of 1 111 680 records each (k_rebase_records and k_check_forest stride over 4096 x 256 lanes) against the fused call

No tolerance, nothing skipped.  Left out: the refusal of 2^24 records in one plane (a plane of 16 M records is at least 8192 x 4096 pixels of speckles:
minutes, not seconds); worlds of more than one GPU over RCCL (the test machines have one; test_config5_strips.py runs a world of one); builds with 64-row
tiles (no such build is shipped); damaged blobs (test_config5_strips.py has them).
"""
import struct
import threading
import time

import numpy as np
import pytest

import strip_planes as sp
import tree_planes as tp
from conftest import check_plane_against_oracle
from test_tree_edges import CONFIGS, SWITCHES

pytestmark = pytest.mark.gpu
FIELDS = ["frame", "ch", "pyr", "level", "cls", "x", "y", "w", "h", "area", "key", "score_strong", "score_weak"]
MASK = 0x09
NONE = 0xFFFFFFFF
MAX_W, MAX_H, MAX_STRIPS = 257, 97, 9
CASES = sp.cases()
KINDS = sorted({k.split("/")[0] for k in CASES})
ACCEPTED = [s for s in range(1, 33) if sp.step_accepted(s)]


def _make(S, cascade_paths, w=MAX_W, h=MAX_H, step=8, min_area=120, mask=MASK):
    f = S.ERFilter(params=S.Params(max_width=w, max_height=h, max_frames=1, thresh_step=step, min_area=min_area, channel_mask=mask))
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    return f


class Rig:
    """An owner and one worker per strip, all at one thresh step and MIN_AREA."""

    def __init__(self, S, cascade_paths, n_workers=MAX_STRIPS, **kw):
        self.owner = _make(S, cascade_paths, **kw)
        self.workers = [_make(S, cascade_paths, **kw) for _ in range(n_workers)]
        self.step, self.min_area, self.mask = self.owner.params.thresh_step, self.owner.params.min_area, self.owner.params.channel_mask

    def set(self, step, min_area):
        for f in self.workers + [self.owner]:
            if step != self.step:
                f.set_thresh_step(step)
            if min_area != self.min_area:
                f.set_min_area(min_area)
        self.step, self.min_area = step, min_area

    def close(self):
        for f in self.workers + [self.owner]:
            f.close()


@pytest.fixture(scope="module")
def rig(S, cascade_paths):
    r = Rig(S, cascade_paths)
    yield r
    r.close()


# ---- the blob, laid out as api_strips.cpp states --------------------------------------------------------------------------------
def _align(x):
    return (x + 255) // 256 * 256


def parse_blob(blob):
    hd = dict(zip(("magic", "version", "w", "h", "strip", "n_strips", "row0", "rows", "n_planes", "thresh_step", "channel_mask", "reserved"),
                  struct.unpack_from("<12I", blob, 0)))
    planes = [dict(zip(("ch", "n_nodes", "n_walls", "start_node", "has_top", "has_bot"), struct.unpack_from("<6I", blob, 48 + 24 * k))) for k in range(hd["n_planes"])]
    at = _align(48 + 24 * len(planes))
    for p in planes:
        p["rec"] = np.frombuffer(blob, np.uint32, 8 * p["n_nodes"], at).reshape(-1, 8)
        at = _align(at + 32 * p["n_nodes"])
    for p in planes:
        for side in ("top", "bot"):
            p[side] = None
            if p["has_" + side]:
                p[side] = np.frombuffer(blob, np.uint32, hd["w"], at)
                at = _align(at + 4 * hd["w"])
    assert at == len(blob)
    return hd, planes


def check_blobs(blobs, six, step, n_strips, mask=MASK):
    """The cut, the phantom rows' layout and k_strip_border_ids from the blobs alone, before any merge."""
    h, w = six[0].shape
    strips = sp.cut_rows(h, n_strips)
    chans = [c for c in range(6) if mask >> c & 1]
    for i, (blob, s) in enumerate(zip(blobs, strips)):
        hd, planes = parse_blob(blob)
        assert (hd["magic"], hd["version"], hd["w"], hd["h"], hd["strip"], hd["n_strips"]) == (0x50525453, 2, w, h, i, n_strips)
        assert (hd["row0"], hd["rows"], hd["thresh_step"], hd["channel_mask"]) == (s.row0, s.rows, step, mask), (i, s)
        assert [p["ch"] for p in planes] == chans
        for p in planes:
            assert (bool(p["has_top"]), bool(p["has_bot"])) == (s.has_top, s.has_bot), (i, s)
            q, hi = tp.quantise(six[p["ch"]], step)
            if s.rows == 0:
                assert p["n_nodes"] == 0 and p["top"] is None and p["bot"] is None
                continue
            assert (p["n_nodes"] == 0) == bool((q[s.r0:s.r1] >= hi).all())
            for side, row in (("top", s.r0), ("bot", s.r1 - 1)):
                ids = p[side]
                if ids is None:
                    continue
                wall = q[row] >= hi
                assert ((ids == NONE) == wall).all(), (i, side)                      # NONE iff the pixel is a wall
                live = ids[~wall]
                assert (live < p["n_nodes"]).all(), (i, side)
                assert ((p["rec"][live, 1] >> 24) == q[row][~wall]).all(), (i, side)  # the record's level byte is the pixel's quantised level


def run_case(S, oracle, oracle_cascades, rig, plane, n_strips, check_oracle=True):
    """Extract each strip in a worker of its own, merge in the owner, compare with the fused call and the oracle.  Returns the merged result."""
    frame = sp.frame_of(plane)
    six = oracle.compute_channels(frame)
    assert (six[0] == plane).all() and (six[3] == 255 - plane).all() and (six[1] == 128).all() and (six[2] == 128).all()
    blobs = [rig.workers[s].strip_extract(frame, s, n_strips) for s in range(n_strips)]
    check_blobs(blobs, six, rig.step, n_strips, rig.mask)
    merged = rig.owner.strip_merge(frame, blobs, want_nodes=True)
    fused = rig.owner.text_detect(frame, want_nodes=True)
    assert merged.cands[FIELDS].tolist() == fused.cands[FIELDS].tolist()
    assert merged.cands.tobytes() == fused.cands.tobytes()
    assert merged.info.tobytes() == fused.info.tobytes()
    assert [p.ch for p in merged.planes] == [c for c in range(6) if rig.mask >> c & 1]
    for pm, pf in zip(merged.planes, fused.planes):
        assert pm.nodes.tobytes() == pf.nodes.tobytes()
        if check_oracle:
            check_plane_against_oracle(oracle, pm, six[pm.ch], oracle_cascades, step=rig.step, min_area=rig.min_area)
    return merged


# ---- the main check -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_area", [120, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_planes_in_strips_give_the_unsplit_result(S, oracle, oracle_cascades, rig, kind, min_area):
    """Every plane of the kind, at every size and strip count it has (strip_planes.cases)."""
    rig.set(8, min_area)
    names = [k for k in CASES if k.split("/")[0] == kind]
    assert names
    for name in names:
        plane, n = CASES[name]
        try:
            run_case(S, oracle, oracle_cascades, rig, plane, n)
        except AssertionError as e:
            raise AssertionError("%s, MIN_AREA %d: %s" % (name, min_area, e)) from e


def test_an_empty_strip_has_no_record_and_no_border_node(S, oracle, rig):
    """empty_strip: the strip of walls has rows, a top and a bottom row, and nothing in them; in the complement channel it is one flat region."""
    rig.set(8, 120)
    plane, n = CASES["empty/65x97/4"]
    frame = sp.frame_of(plane)
    hd, planes = parse_blob(rig.workers[1].strip_extract(frame, 1, n))
    assert hd["rows"] == 32 and planes[0]["n_nodes"] == 0 and planes[0]["n_walls"] >= 32 * 65 and planes[0]["start_node"] == NONE
    assert (planes[0]["top"] == NONE).all() and (planes[0]["bot"] == NONE).all()
    # channel 3: 255 - 255 = 0 everywhere, one flat region of level 0 (a record for each of the two tiles it lies in)
    rec = planes[1]["rec"]
    assert 1 <= planes[1]["n_nodes"] <= 2 and (rec[:, 1] >> 24 == 0).all()
    assert (planes[1]["top"] != NONE).all() and (planes[1]["bot"] != NONE).all() and set(planes[1]["top"].tolist()) == set(planes[1]["bot"].tolist())


def test_all_six_channels(S, oracle, oracle_cascades, cascade_paths):
    """channel_mask 0x3F: the plane, its complement and four flat chroma planes (Cr = Cb = 128 and their complements) in every blob."""
    r = Rig(S, cascade_paths, n_workers=4, mask=0x3F)
    for min_area in (120, 1):
        r.set(8, min_area)
        for plane, n in ((sp.serpent(257, 97, 4), 4), (sp.rings(257, 65, 3, 8), 3), (sp.wall_cut(65, 33, 2, "below"), 2), (sp.empty_strip(255, 96, 3), 3)):
            run_case(S, oracle, oracle_cascades, r, plane, n)
    r.close()


# ---- thresh steps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", ACCEPTED)
def test_every_accepted_thresh_step(S, oracle, oracle_cascades, rig, step):
    """rings (as deep as the step has levels), serpent, levels_across and wall_cut at a step the sentinel rule accepts, MIN_AREA 120 and 1."""
    for min_area in (120, 1):
        rig.set(step, min_area)
        for name, (plane, n) in sp.step_cases(step).items():
            try:
                run_case(S, oracle, oracle_cascades, rig, plane, n)
            except AssertionError as e:
                raise AssertionError("step %d, %s, MIN_AREA %d: %s" % (step, name, min_area, e)) from e


@pytest.mark.parametrize("step", [1, 3, 6])
def test_a_refused_step_is_refused_where_a_strip_has_rows_above_it(S, oracle, oracle_cascades, cascade_paths, step):
    """No sentinel level: STR_ER_EINVAL naming thresh_step from strip 1, while strip 0 of the same context extracts; after set_thresh_step(8) the same
    contexts extract and merge correctly."""
    assert not sp.step_accepted(step)
    r = Rig(S, cascade_paths, n_workers=2, w=65, h=65, step=step)
    plane = sp.serpent(65, 65, 2)
    frame = sp.frame_of(plane)
    for f in r.workers:
        with pytest.raises(S.StrErError) as e:
            f.strip_extract(frame, 1, 2)
        assert e.value.code == -1 and "thresh_step" in str(e.value)
        hd, planes = parse_blob(f.strip_extract(frame, 0, 2))
        assert (hd["rows"], hd["thresh_step"]) == (32, step) and planes[0]["n_nodes"] > 0 and planes[0]["has_bot"] == 1
        with pytest.raises(S.StrErError):
            f.strip_extract_dev(frame, 1, 2)
    r.set(8, 120)
    run_case(S, oracle, oracle_cascades, r, plane, 2)
    run_case(S, oracle, oracle_cascades, r, sp.rings(65, 65, 2, 8), 2)
    r.close()


# ---- kernel configurations ------------------------------------------------------------------------------------------------------
def _small_planes(w, h, n):
    out = {"bar": sp.bar(w, h, n), "flat": sp.flat(w, h, n), "stripes": sp.stripes(w, h, n), "serpent": sp.serpent(w, h, n), "u": sp.u_shape(w, h, n),
           "u_mirror": sp.u_shape(w, h, n, mirror=True), "u_three": sp.u_shape(w, h, n, three=True), "rings": sp.rings(w, h, n, 8),
           "rings_wall": sp.rings(w, h, n, 8, wall_ring=20), "levels": sp.levels_across(w, h, n), "corner": sp.corner(w, h, n), "corner_b": sp.corner(w, h, n, "b"),
           "empty": sp.empty_strip(w, h, n), "empty_inverted": 255 - sp.empty_strip(w, h, n)}
    for kind in ("above", "below", "both"):
        out["wall_" + kind] = sp.wall_cut(w, h, n, kind)
    return out


@pytest.mark.parametrize("w, h, n", [(65, 65, 3), (257, 97, 4)])
def test_node_tables_are_the_same_under_every_kernel_configuration(S, oracle, oracle_cascades, cascade_paths, monkeypatch, w, h, n):
    """A strip's groups of tiles start at its phantom row and are not aligned with the whole plane's: the grouping kernels see other groups for the same
    pixels.  Every builder at one size (65 x 65 in 3 strips; 257 x 97 in 4: five tile columns, so a 4 x 4 group and a remainder) under every entry of
    test_tree_edges.CONFIGS, set on workers and owner alike, at MIN_AREA 120 and 1."""
    planes = _small_planes(w, h, n)
    for min_area in (120, 1):
        ref = None
        for cfg, env in CONFIGS.items():
            for k in SWITCHES:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            r = Rig(S, cascade_paths, n_workers=n, w=w, h=h, min_area=min_area)
            got = {}
            for name, plane in planes.items():
                try:
                    m = run_case(S, oracle, oracle_cascades, r, plane, n, check_oracle=ref is None)
                except AssertionError as e:
                    raise AssertionError("%s under %s, MIN_AREA %d: %s" % (name, cfg, min_area, e)) from e
                got[name] = (m.cands.tobytes(), m.info.tobytes(), [p.nodes.tobytes() for p in m.planes])
            r.close()
            if ref is None:
                ref = got
            assert got == ref, cfg


# ---- other entry points ---------------------------------------------------------------------------------------------------------
def test_device_blobs_and_plane_select(S, oracle, oracle_cascades, rig):
    rig.set(8, 1)
    n = 4
    plane = sp.serpent(257, 97, n)
    plane[:, 100:103] = sp.MID                                     # ... and a bar of another level through all strips
    frame = sp.frame_of(plane)
    fused = rig.owner.text_detect(frame, want_nodes=True)
    # blobs that stay on the device: each in its worker's buffer, merged from there
    dev = [rig.workers[s].strip_extract_dev(frame, s, n) for s in range(n)]
    host = [rig.workers[s].strip_extract(frame, s, n) for s in range(n)]
    assert [b for _, b in dev] == [len(x) for x in host]
    dev = [rig.workers[s].strip_extract_dev(frame, s, n) for s in range(n)]
    merged = rig.owner.strip_merge_ex(frame, [p for p, _ in dev], [b for _, b in dev], device_blobs=True, want_nodes=True)
    assert merged.cands.tobytes() == fused.cands.tobytes() and merged.info.tobytes() == fused.info.tobytes()
    six = oracle.compute_channels(frame)
    for pm, pf in zip(merged.planes, fused.planes):
        assert pm.nodes.tobytes() == pf.nodes.tobytes()
        check_plane_against_oracle(oracle, pm, six[pm.ch], oracle_cascades, step=8, min_area=1)
    # channel 3 alone: the fused call's records of that channel
    part = rig.owner.strip_merge_ex(frame, host, plane_select=np.array([0, 1], np.uint8), want_nodes=True)
    want = fused.cands[fused.cands["ch"] == 3]
    assert part.cands[FIELDS].tolist() == want[FIELDS].tolist() and len(part.planes) == 1 and part.planes[0].ch == 3
    assert part.planes[0].nodes.tobytes() == fused.planes[1].nodes.tobytes()
    check_plane_against_oracle(oracle, part.planes[0], six[3], oracle_cascades, step=8, min_area=1)


def test_detect_frame_strips_with_ranks_that_hold_empty_strips(S, cascade_paths):
    """40 rows are two tile rows: of four ranks, 0 and 2 hold strips without rows, and the one cut lies between ranks 1 and 3."""
    w, h, world = 257, 40, 4
    assert [s.rows for s in sp.cut_rows(h, world)] == [0, 32, 0, 8]
    plane = sp.rings(w, h, world, 8)                                # 31 rings around a centre on the cut: the pool is not empty
    frame = sp.frame_of(plane)
    f = _make(S, cascade_paths, w, h, min_area=1)
    fused = f.text_detect(frame)
    f.close()
    comms = S.Comm.local_group(world)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            g = _make(S, cascade_paths, w, h, min_area=1)
            out[r] = S.dist.detect_frame_strips(g, comms[r], frame)
            g.close()
        except Exception as e:                                       # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert not errs, errs
    assert len(fused.cands) > 0
    for r in range(world):
        assert out[r] is not None and out[r][FIELDS].tolist() == fused.cands[FIELDS].tolist(), r


# ---- stages ---------------------------------------------------------------------------------------------------------------------
def test_strip_merge_with_track_and_group_stages(S, cascade_paths):
    """stage_rules.h allows er_track / er_grouping on a strip merge of ALL planes: the lines of an S-text frame put together from 3 strips are text_detect's."""
    w, h, n = 640, 480, 3
    frame = S.synth.stext_bgr(S.synth.frame_seed(12), w, h)
    stages = S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP
    owner = _make(S, cascade_paths, w, h, mask=0x3F)
    workers = [_make(S, cascade_paths, w, h, mask=0x3F) for _ in range(n)]
    blobs = [workers[s].strip_extract(frame, s, n) for s in range(n)]
    merged = owner.strip_merge(frame, blobs, stages=stages)
    fused = owner.text_detect(frame, stages)
    for name in ("info", "cands", "tracks", "texts", "text_ers", "group_bounds", "group_all"):
        a, b = getattr(merged, name), getattr(fused, name)
        assert a is not None and b is not None, name
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), name
    assert len(fused.texts) > 0 and len(merged.texts) == len(fused.texts)
    for f in workers + [owner]:
        f.close()


# ---- past one grid round --------------------------------------------------------------------------------------------------------
def test_a_strip_of_more_records_than_one_grid_round(S, cascade_paths):
    """k_rebase_records and k_check_forest are launched with at most 4096 workgroups of 256 lanes: strips of 32 x 36 tiles with 965 exported nodes each
    (1 111 680 records a strip, counted from the blobs' headers) take their grid-stride loops into a second round -- the top strip as the first of
    the plane's records, the bottom one with ids, keys and rows that the second round has to move as well; every tile has a kept region, so whichever
    tiles hold the ids past 2^20 show in the node table.  Against the fused call only: the oracle on 2048 x 2304 pixels is not a matter of seconds."""
    plane = sp.big_strips_plane()
    h, w = plane.shape
    frame = sp.frame_of(plane)
    t0 = time.perf_counter()
    owner = _make(S, cascade_paths, w, h, mask=1)
    worker = _make(S, cascade_paths, w, h, mask=1)
    blobs = [worker.strip_extract(frame, s, 2) for s in range(2)]
    worker.close()
    per_strip = sp.BIG_TILES_X * sp.BIG_TILE_ROWS * sp.BIG_TILE_NODES
    for i, blob in enumerate(blobs):
        hd, planes = parse_blob(blob)
        assert (hd["row0"], hd["rows"]) == ((0, 1152), (1152 - 32, 1152))[i]
        assert planes[0]["n_nodes"] == per_strip > 1 << 20
    merged = owner.strip_merge(frame, blobs, want_nodes=True)
    t1 = time.perf_counter()
    fused = owner.text_detect(frame, want_nodes=True)
    t2 = time.perf_counter()
    print("big strips: extract + merge %.2f s, fused %.2f s" % (t1 - t0, t2 - t1))
    assert merged.cands.tobytes() == fused.cands.tobytes() and merged.info.tobytes() == fused.info.tobytes()
    assert merged.planes[0].nodes.tobytes() == fused.planes[0].nodes.tobytes()
    n_tiles = 2 * sp.BIG_TILES_X * sp.BIG_TILE_ROWS
    assert merged.planes[0].n_created == fused.planes[0].n_created == n_tiles * (sp.BIG_TILE_NODES - 1) + 1       # the speckles and blocks of every tile, and the ground
    assert merged.planes[0].n_kept == n_tiles + 1                                                                    # every tile's block, and the ground
    lab, _ = tp.ndimage.label(sp.big_tile() <= sp.MID)                     # the block and the speckles that touch it: where it lies in its tile
    sl = tp.ndimage.find_objects(lab)[int(np.argmax(np.bincount(lab.ravel())[1:]))]
    boxes = sorted((int(a["y"]), int(a["x"])) for a in merged.planes[0].nodes if int(a["area"]) < 1000)
    assert boxes == sorted((32 * ty + sl[0].start, 64 * tx + sl[1].start) for ty in range(2 * sp.BIG_TILE_ROWS) for tx in range(sp.BIG_TILES_X))
    owner.close()
