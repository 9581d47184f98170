"""k_group_bins: every group of tiles of a large text-like batch joined in the smallest k_group_merge table that holds its records.

The CPU half pins, with the census of tests/tree_planes.py, the planes the GPU half runs -- groups of exactly 512 / 1024 / 2048 / 2528 records and of one
more, under the 8 x 4 groups of a batch of more than 96 planes -- and the premise of the whole change: 8 x 4 groups of the luma pyramid of S-text frames
hold more than 2048 records (and none more than 2528).  The GPU half checks the trees against the oracle, `last_tree_stats()["records"]` and
`last_group_stats()` against the census -- the counter that says which way a group went --, and the developer switches against one another, byte for
byte: STR_ER_GROUP_GRID (one or two workgroups walk every list), STR_ER_GROUP_BINS=4 / 2 (a list of its own for the 2048-record table; the 512- and the
2528-record table alone; the default leaves the groups of up to 2048 records to the 2528-record table), STR_ER_GROUP_BINS=0 (the launches per class of plane).
"""
import numpy as np
import pytest

import tree_planes as tp
from conftest import check_plane_against_oracle

TABLES = (512, 1024, 2048, 2528)
DEFAULT_TABLES = (512, 1024, 2528)
GX, GY = 8, 4                 # the groups of a text-like batch of more than 96 planes
SWITCHES = ("STR_ER_TILE_KERNEL", "STR_ER_TILE2", "STR_ER_GROUPS", "STR_ER_GROUP_X", "STR_ER_GROUP_Y", "STR_ER_GROUP_KERNEL", "STR_ER_GROUP_BINS", "STR_ER_GROUP_GRID")
SPARSE = {"STR_ER_TILE_KERNEL": "sparse", "STR_ER_TILE2": "0"}


def cap_planes():
    return {(cap, extra): tp.cap_plane(GX, GY, cap, extra) for cap in TABLES for extra in (0, 1)}


_CENSUS = {}


def _census(p, min_area=1):
    key = (p.shape, min_area, p.tobytes())
    if key not in _CENSUS:
        _CENSUS[key] = tp.Census(p, 8, min_area)
    return _CENSUS[key]


def expected_stats(planes, tables=DEFAULT_TABLES, min_area=1):
    """What last_group_stats() must say for one call of these planes: every group of at least two tiles in the smallest table that holds its records."""
    per = {t: 0 for t in TABLES}
    listed = one_tile = 0
    for p in planes:
        c = _census(p, min_area)
        g = c.group_records(GX, GY, tp.SPARSE_FOLD)
        for iy in range(g.shape[0]):
            for ix in range(g.shape[1]):
                if min(GX, c.tiles_x - ix * GX) * min(GY, c.tiles_y - iy * GY) < 2:
                    one_tile += 1
                    continue
                fits = [t for t in tables if g[iy, ix] <= t]
                if fits: per[fits[0]] += 1
                else: listed += 1
    return {"per_table": per, "listed": listed, "one_tile": one_tile}


# =================================================================================================================================
# CPU
# =================================================================================================================================
def test_cap_planes_hold_cap_and_cap_plus_one_records_in_8x4_groups():
    for (cap, extra), p in cap_planes().items():
        c = _census(p)
        assert p.shape == (128, 1536)
        assert (c.exported(tp.SPARSE_FOLD) == c.nodes()).all(), (cap, extra)       # MIN_AREA 1: records a tile = nodes a tile
        g = c.group_records(GX, GY, tp.SPARSE_FOLD)
        assert g.shape == (1, 3) and int(g[0, 1]) == cap + extra, (cap, extra)
        assert int(g[0, 0]) == int(g[0, 2]) == 32 * (cap // 160), (cap, extra)     # the neighbours: a fifth, in whole tiles
        assert int(c.nodes().max()) <= 256, (cap, extra)                           # no tile near a tile kernel's limit
    # 16 neighbours and the middle groups of 512 + 0; 512 + 1 and 1024 + 0; 1024 + 1 and 2048 + 0; 2048 + 1 and 2528 + 0; 2528 + 1
    assert expected_stats(cap_planes().values(), TABLES) == {"per_table": {512: 17, 1024: 2, 2048: 2, 2528: 2}, "listed": 1, "one_tile": 0}
    assert expected_stats(cap_planes().values()) == {"per_table": {512: 17, 1024: 2, 2048: 0, 2528: 4}, "listed": 1, "one_tile": 0}


def test_luma_pyramid_groups_of_text_frames_overflow_the_2048_table(S, oracle):
    """The premise: 8 x 4 groups of levels 3-4 of the luma pyramid of 1080p S-text frames 0-2 hold 2118; 2206 and 2271; 2167 and 2246 records -- more than
    k_group_merge<2048, 1024> holds, none more than the 2528-record table does."""
    over = {}
    for i in range(3):
        luma = oracle.compute_channels(S.synth.stext_bgr(S.synth.frame_seed(i), 1920, 1080))[0]
        for p in oracle.pyramid(luma, 5)[3:]:
            assert p.shape in ((382, 679), (270, 480))
            g = tp.Census(p, 8, 120).group_records(GX, GY, tp.SPARSE_FOLD).ravel()
            assert int(g.max()) <= 2528, i
            over.setdefault(i, []).extend(int(x) for x in g if x > 2048)
    assert sum(len(v) for v in over.values()) >= 1
    assert {i: sorted(v) for i, v in over.items()} == {0: [2118], 1: [2206, 2271], 2: [2167, 2246]}


# =================================================================================================================================
# GPU
# =================================================================================================================================
def _context(S, monkeypatch, env, planes, min_area=1):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    w, h = max(p.shape[1] for p in planes), max(p.shape[0] for p in planes)
    return S.ERFilter(params=S.Params(max_width=w, max_height=h, max_frames=-(-len(planes) // 6), thresh_step=8, min_area=min_area))


def _call(S, monkeypatch, env, planes):
    f = _context(S, monkeypatch, env, planes)
    r = f.detect_planes_list(planes, S.STAGE_EXTRACT | S.STAGE_NMS, want_nodes=True)
    out = (r, f.last_tree_stats()["records"], f.last_group_stats())
    f.close()
    return out


def _same(a, b, what):
    assert a.info.tobytes() == b.info.tobytes() and a.cands.tobytes() == b.cands.tobytes(), what
    assert len(a.planes) == len(b.planes), what
    for i, (pa, pb) in enumerate(zip(a.planes, b.planes)):
        assert pa.nodes.tobytes() == pb.nodes.tobytes(), (what, i)


@pytest.fixture(scope="module")
def cap_call(S, oracle):
    """The eight cap planes thirteen times over: 104 planes of 1536 x 128 in one call, on the default path."""
    mp = pytest.MonkeyPatch()
    planes = list(cap_planes().values()) * 13
    try:
        yield planes, _call(S, mp, SPARSE, planes)
    finally:
        mp.undo()


@pytest.mark.gpu
def test_groups_at_every_table_and_one_above(S, oracle, cap_call):
    planes, (r, records, stats) = cap_call
    assert len(planes) == 104
    for p, x in zip(planes[:8], r.planes[:8]):
        check_plane_against_oracle(oracle, x, p, step=8, min_area=1)
    for i, x in enumerate(r.planes[8:], 8):
        assert x.nodes.tobytes() == r.planes[i % 8].nodes.tobytes() and x.n_created == r.planes[i % 8].n_created, i
    assert records == sum(_census(p).records(tp.SPARSE_FOLD) for p in planes)
    e = expected_stats(planes)
    assert stats == e
    assert stats["listed"] == 13 == sum(int((_census(p).group_records(GX, GY, tp.SPARSE_FOLD) > 2528).sum()) for p in planes)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", ["1", "2"])
def test_one_or_two_workgroups_walk_every_list(S, monkeypatch, cap_call, grid):
    """221 / 26 / 52 groups per list and one or two workgroups per launch: the grid-stride loop of k_group_merge_list, its LDS tables used again and again."""
    planes, (ref, records, stats) = cap_call
    r, rec2, st2 = _call(S, monkeypatch, dict(SPARSE, STR_ER_GROUP_GRID=grid), planes)
    _same(ref, r, grid)
    assert (rec2, st2) == (records, stats)


@pytest.mark.gpu
def test_four_tables_two_tables_and_the_launches_per_class_of_plane_give_the_same(S, monkeypatch, cap_call):
    planes, (ref, records, stats) = cap_call
    assert stats["per_table"] == {512: 221, 1024: 26, 2048: 0, 2528: 52}
    r, rec2, st2 = _call(S, monkeypatch, dict(SPARSE, STR_ER_GROUP_BINS="4"), planes)
    _same(ref, r, "four tables")
    assert rec2 == records and st2 == expected_stats(planes, TABLES) and st2["per_table"] == {512: 221, 1024: 26, 2048: 26, 2528: 26}
    r, rec2, st2 = _call(S, monkeypatch, dict(SPARSE, STR_ER_GROUP_BINS="2"), planes)
    _same(ref, r, "two tables")
    assert rec2 == records and st2 == expected_stats(planes, (512, 2528)) and st2["per_table"] == {512: 221, 1024: 0, 2048: 0, 2528: 78}
    r, rec2, st2 = _call(S, monkeypatch, dict(SPARSE, STR_ER_GROUP_BINS="0"), planes)
    _same(ref, r, "per class of plane")
    # (one table per class of plane: what it lists depends on the class -- at least every group no table holds)
    assert rec2 == records and st2["per_table"] == {t: 0 for t in TABLES} and st2["one_tile"] == 0 and st2["listed"] >= stats["listed"]


@pytest.mark.gpu
def test_text_batch_with_and_without_bins_and_twice_on_one_context(S, oracle, cascade_paths, monkeypatch):
    """Five 640 x 360 S-text frames at pyr3x8 (120 planes): every output array is the same with the launches per class of plane, and the same again when
    the context runs the batch a second time -- then with the grids sized from the first run's lists."""
    W, H = 640, 360
    frames = np.stack([S.synth.stext_bgr(S.synth.frame_seed(40 + i), W, H) for i in range(5)])
    out = {}
    for bins in ("1", "0"):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("STR_ER_GROUP_BINS", bins)
        f = S.ERFilter(params=S.Params(max_width=W, max_height=H, max_frames=5, n_pyr_levels=8, channel_mask=0x07))
        f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
        out[bins] = []
        for _ in range(2):
            out[bins].append((f.text_detect(frames, want_nodes=True), f.last_tree_stats()["records"], f.last_group_stats()))
        f.close()
    (a, rec_a, st_a), (a2, rec_a2, st_a2) = out["1"]
    assert len(a.planes) == 120 and len(a.cands) > 0
    _same(a, a2, "second run")
    assert (rec_a, st_a) == (rec_a2, st_a2)
    for b, rec_b, st_b in out["0"]:
        _same(a, b, "bins off")
        assert rec_b == rec_a and st_b["per_table"] == {t: 0 for t in TABLES}
    n_groups = 0
    for lv in range(8):
        w, h = oracle.pyr_dims(W, H, lv)
        n_groups += 3 * 5 * (-(-(-(-w // tp.TILE_W)) // GX)) * (-(-(-(-h // tp.TILE_H)) // GY))
    assert sum(st_a["per_table"].values()) + st_a["listed"] + st_a["one_tile"] == n_groups
    assert st_a["listed"] == 0 and st_a["one_tile"] > 0          # (the small levels of the pyramid are one tile)


def _shape_planes():
    """Remainder groups, tiles of walls at a group's corner / first tile / middle, flat planes (tests/test_tree_edges.py: group_shape_cases), planes whose
    last group is ONE tile under 8 x 4 groups, and a plane of 401 records a tile: a fresh context runs out of node records on it -- its tiles have no
    records of their own (tile_nbase NONE) in the first attempt of the call -- and, once the call has grown them, its one group holds 12 832."""
    W = 0
    cases = {
        "remainders 5x5": tp.group_plane(5, 5, [[3 + x + 5 * y for x in range(5)] for y in range(5)]),
        "one tile wide": tp.group_plane(1, 6, [[2], [3], [4], [5], [6], [7]]),
        "one tile high": tp.group_plane(6, 1, [[2, 3, 4, 5, 6, 7]]),
        "walls at a group's corner": tp.group_plane(8, 4, [[2] * 8, [2] * 8, [2] * 8, [2, 2, 2, 2, 2, 2, 2, W]]),
        "walls at a group's first tile": tp.group_plane(8, 4, [[2, 2, 2, 2, W, 2, 2, 2], [2] * 8, [2] * 8, [2] * 8]),
        "walls in a group's middle": tp.group_plane(4, 4, [[2] * 4, [2, W, 2, 2], [2, 2, W, 2], [2] * 4]),
        "flat 8x4": np.full((4 * tp.TILE_H, 8 * tp.TILE_W), tp.BG, np.uint8),
        "nine tiles wide": tp.group_plane(9, 1, [[2, 3, 4, 5, 6, 7, 8, 9, 10]]),
        "five tiles high": tp.group_plane(1, 5, [[2], [3], [4], [5], [6]]),
        "401 records a tile": tp.lattice_plane(8 * tp.TILE_W, 4 * tp.TILE_H, 400),
    }
    return cases


def test_shape_planes_hold_one_tile_groups_walls_and_a_group_no_table_holds():
    cases = _shape_planes()
    e = expected_stats(cases.values())
    assert e["one_tile"] == 2 and e["listed"] == 1
    assert sum(e["per_table"].values()) == e["per_table"][512] == 2 + 2 + 1 + 1 + 1 + 1 + 1 + 1 + 1
    c = _census(cases["401 records a tile"])
    assert c.group_records(GX, GY, tp.SPARSE_FOLD).tolist() == [[32 * 401]] and c.records(tp.SPARSE_FOLD) > 0.06 * 8 * 4 * 2048
    assert _census(cases["walls at a group's corner"]).tiles[3, 7].nodes == 0 and _census(cases["walls at a group's first tile"]).tiles[0, 4].nodes == 0


@pytest.mark.gpu
def test_group_shapes_under_the_bins(S, oracle, monkeypatch):
    cases = _shape_planes()
    planes = list(cases.values()) * 10          # 100 planes
    r, records, stats = _call(S, monkeypatch, SPARSE, planes)
    for (name, p), x in zip(cases.items(), r.planes):
        check_plane_against_oracle(oracle, x, p, step=8, min_area=1)
    n = len(cases)
    for i, x in enumerate(r.planes[n:], n):
        assert x.nodes.tobytes() == r.planes[i % n].nodes.tobytes(), i
    assert records == sum(_census(p).records(tp.SPARSE_FOLD) for p in planes)
    assert stats == expected_stats(planes) and stats["one_tile"] == 20 and stats["listed"] == 10
    r0, rec0, st0 = _call(S, monkeypatch, dict(SPARSE, STR_ER_GROUP_BINS="0"), planes)
    _same(r, r0, "bins off")
    assert rec0 == records
