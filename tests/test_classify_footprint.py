"""k_classify's batch build -- 32 candidates on 4 waves, a grid sized from the context's previous batch -- and k_cand_records, against the oracle.

Every GPU test runs a batch of 97 planes, one more than SPEC_PLANES = 96, so launch_classify takes the batch build
(k_classify<32, 4>, er_classify.inl) and not k_classify<16, 16>.  The cascades are the made-up families of tests/cascade_cases.py, tuned on
the candidates of the 97 small planes of test_classify_edges.py (15 539 of them); all comparisons are `==` against the oracle on cls, both
scores, n_strong and n_weak (check_plane_against_oracle): the kernel adds a stage's stump outputs in file order, whichever wave sums it.

  pool sizes      PER - 1, PER, PER + 1 and 2 PER + 1 = 31, 32, 33, 65 candidates in the WHOLE batch: 96 constant planes, which pool nothing,
                  and one plane of exactly that many; the stage-parallel form (small_par) and lane_cascade_generic (small_generic)
  forced grids    STR_ER_CLASSIFY_GRID = 1 and 2: a workgroup goes round its loop 486 / 243 times; the same with the two
                  forms that lost on the line and stay as developer switches (STR_ER_CLASSIFY_FORM = 8: 32 candidates on 8 waves, 64: 64 on 8)
  the hint        one context, batches that pool 174, 15 539, 0 and 15 539 candidates: the grid -- ceil(previous / 32) plus an eighth plus 8,
                  at most 1024 -- is 14 workgroups for 486 rounds of candidates, then 554 for none, then the full grid (no hint after an empty batch)
  stage lengths   len_0_par, len_1_par: stages of 0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129 and 200 stumps around the 64-stump chunk a wave
                  stages in LDS, as the strong and as the weak cascade; 16 stage jobs for 4 waves
  many stumps     path_8+8 (4776 stumps) and path_4777: unit dirs, so both take the stage-parallel form now -- no table bounds it
  no cascades     STAGE_EXTRACT | STAGE_NMS: k_cand_records writes the records: the oracle's pool, cls 0, score_strong -DBL_MAX, score_weak 0
"""
import numpy as np
import pytest

import cascade_cases as cc
from conftest import check_plane_against_oracle
from test_classify_edges import World, expected_path

PER = 32            # CLS_BATCH_PER (er_classify.inl)
N_PLANES = 97
POOL_SIZES = [PER - 1, PER, PER + 1, 2 * PER + 1]


def tuned(world, name):
    """((strong, weak), the oracle's pair): the small pair tuned on the batch's own 15 539 candidates, the long families on the rectangle plane's
    1140 as in test_classify_edges.py (the numpy model that tunes them holds candidates x stumps doubles)"""
    which = "batch97" if name.startswith("small") else "rect"
    return world.family(name, which), world.oracle_cascades(name, which)


@pytest.fixture(scope="module")
def world(oracle, tmp_path_factory):
    return World(oracle, tmp_path_factory.mktemp("footprint_cascades"))


def _filter(S, w=64, h=64):
    return S.ERFilter(params=S.Params(thresh_step=8, min_area=0, max_area=900000, stability_t=0, overlap_coef=0.7, max_width=w, max_height=h,
                                      max_frames=17))


def _load(f, world, name):
    (strong, weak), ocs = tuned(world, name)
    f.load_cascade_text(0, strong.text())
    f.load_cascade_text(1, weak.text())
    assert f.cascade_info(0) == strong.shape and f.cascade_info(1) == weak.shape
    return ocs


def _check_batch(oracle, f, planes, ocs, stages=None):
    res = f.detect_planes(np.stack(planes), want_nodes=True) if stages is None else f.detect_planes(np.stack(planes), stages, want_nodes=True)
    assert len(res.planes) == len(planes)
    for p, img in zip(res.planes, planes):
        check_plane_against_oracle(oracle, p, img, ocs, **cc.RECT_PRM)
    return res


@pytest.fixture(scope="module")
def batch97(world):
    planes, _ = world.planes("batch97")
    assert len(planes) == N_PLANES
    return planes


# ======== CPU: the inputs are what the GPU tests claim ===============================================================================
def test_the_planes_pool_what_the_cases_need(world, oracle, batch97):
    """A constant plane pools nothing, count_plane(n) exactly n, and the 97 small planes 15 539: 486 rounds of 32."""
    assert len(cc.pool_of(oracle, np.full((96, 128), 200, np.uint8))[0]) == 0
    assert len(cc.pool_of(oracle, np.full((64, 64), 200, np.uint8))[0]) == 0
    assert [len(cc.pool_of(oracle, cc.count_plane(oracle, n))[0]) for n in POOL_SIZES] == POOL_SIZES
    pools = [len(cc.pool_of(oracle, p)[0]) for p in batch97]
    assert sum(pools) == 15539 and pools[0] == 174
    assert -(-pools[0] // PER) + (-(-pools[0] // PER)) // 8 + 8 == 14 and -(-sum(pools) // PER) == 486


@pytest.mark.parametrize("name,path", [("small_par", "par"), ("small_generic", "generic"), ("len_0_par", "par"), ("len_1_par", "par"),
                                       ("path_8+8", "par"), ("path_4777", "generic")])
def test_the_families_on_the_batch(world, oracle, batch97, name, path):
    """The families' shapes, and every class among the batch's candidates (oracle); `path` is what k_classify's selection was before the
    table left LDS (expected_path of test_classify_edges.py states that rule) -- path_4777 has unit dirs only and is stage-parallel now."""
    (strong, weak), ocs = tuned(world, name)
    assert expected_path(strong, weak) == path
    if name.startswith("len"):
        assert (strong if name == "len_0_par" else weak).stage_n == cc.STAGE_LENGTHS
        assert len(strong.stage_n) + len(weak.stage_n) == 16
    if name.startswith("path"):
        assert len(strong.rows) + len(weak.rows) == (4777 if name == "path_4777" else 4776)
        assert all(r[2] in (1, -1) for r in strong.rows + weak.rows)
    cls = np.concatenate([oracle.classify(p, cc.pool_of(oracle, p)[0], *ocs)[0] for p in batch97])
    shares = [float((cls == k).mean()) for k in (0, 1, 2)]
    print(f"{name} on the 97 planes: cls 0/1/2 {[round(v, 3) for v in shares]}")
    assert len(cls) == 15539 and min(shares) > 0.01, shares           # (every class is there in numbers: 155 candidates at the least)


# ======== GPU ========================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["par", "generic"])
def test_pool_sizes_around_the_workgroup(S, world, oracle, form):
    """31, 32, 33 and 65 candidates in a batch of 97 planes: 96 constant planes and one that pools exactly so many, in the middle."""
    f = _filter(S, 128, 96)
    try:
        ocs = _load(f, world, "small_" + form)
        for n in POOL_SIZES:
            planes = [np.full((96, 128), 200, np.uint8) for _ in range(N_PLANES)]
            planes[50] = cc.count_plane(oracle, n)
            res = _check_batch(oracle, f, planes, ocs)
            assert sum(p.n_pool for p in res.planes) == n == res.planes[50].n_pool
    finally:
        f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("grid,form", [(1, 0), (2, 0), (0, 8), (1, 8), (0, 64), (1, 64)])
def test_forced_grids(S, world, oracle, batch97, monkeypatch, grid, form):
    """One and two workgroups for 15 539 candidates: the loop of a workgroup goes round hundreds of times, rows, chunks and stage sums reused each
    time.  form 8 and 64: the other two batch builds."""
    if grid:
        monkeypatch.setenv("STR_ER_CLASSIFY_GRID", str(grid))
    if form:
        monkeypatch.setenv("STR_ER_CLASSIFY_FORM", str(form))
    f = _filter(S)
    try:
        _check_batch(oracle, f, batch97, _load(f, world, "small_par"))
        if grid == 1:
            _check_batch(oracle, f, batch97, _load(f, world, "small_generic"))
            res = _check_batch(oracle, f, batch97, None, S.STAGE_EXTRACT | S.STAGE_NMS)           # (k_cand_records on one workgroup)
            assert all(int(c["cls"]) == 0 for p in res.planes for c in p.cands)
    finally:
        f.close()


@pytest.mark.gpu
def test_the_grid_hint_is_only_a_hint(S, world, oracle, batch97):
    """One context, four batches in a row that pool 174, 15 539, 0 and 15 539 candidates: the second is launched with 14 workgroups, the third
    with 554, the fourth with the full grid."""
    blank = np.full((64, 64), 200, np.uint8)
    few = [batch97[0]] + [blank] * (N_PLANES - 1)
    f = _filter(S)
    try:
        ocs = _load(f, world, "small_par")
        for planes, total in ((few, 174), (batch97, 15539), ([blank] * N_PLANES, 0), (batch97, 15539)):
            res = _check_batch(oracle, f, planes, ocs)
            assert sum(p.n_pool for p in res.planes) == total
    finally:
        f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["len_0_par", "len_1_par", "path_8+8", "path_4777"])
def test_stage_lengths_and_many_stumps(S, world, oracle, batch97, name):
    """len_*: stages of 0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129 and 200 stumps through the 64-stump chunks, 16 stage jobs dealt to 4 waves.
    path_*: 4776 and 4777 stumps on the stage-parallel form."""
    f = _filter(S)
    try:
        res = _check_batch(oracle, f, batch97, _load(f, world, name))
        assert sum(p.n_strong for p in res.planes) > 0 and sum(p.n_weak for p in res.planes) > 0
    finally:
        f.close()


@pytest.mark.gpu
def test_records_without_the_cascades(S, world, oracle, batch97):
    """STAGE_EXTRACT | STAGE_NMS on the batch: the records of the oracle's pool with cls 0, score_strong -DBL_MAX and score_weak 0, nothing
    counted strong or weak; then STAGE_ALL on the same context gives the oracle's classes again."""
    f = _filter(S)
    try:
        ocs = _load(f, world, "small_par")
        res = _check_batch(oracle, f, batch97, None, S.STAGE_EXTRACT | S.STAGE_NMS)
        assert sum(p.n_pool for p in res.planes) == 15539
        for p in res.planes:
            assert p.n_strong == 0 and p.n_weak == 0 and len(p.cands) == p.n_pool
            assert all(int(c["cls"]) == 0 and float(c["score_strong"]) == -cc.DBL_MAX and float(c["score_weak"]) == 0.0 for c in p.cands)
        _check_batch(oracle, f, batch97, ocs, S.STAGE_ALL)
    finally:
        f.close()
