"""er_track, er_grouping's GPU half and calc_color at the kernels' own edges (track_kernels.hip).

Every input below is made up for one property of a kernel: a clause of a rule exactly at equality, a closure many generations
deep or wider than the workgroup, a count on either side of a 256-lane chunk, a pair list larger than its first buffer, more
images than k_pair_prefix takes in one chunk, the box forms of color_rows, a full big-box queue.  The CPU section proves on the
oracle alone that each input has the property it was made for; the GPU section compares the HIP path with the oracle, `==`."""
import functools
import types

import numpy as np
import pytest

from oracle.oracle import Oracle
from test_track import _check_lines, _expected_tracks, _ycrcb

ER = Oracle.ER_DTYPE
ECAPACITY = -7                 # STR_ER_ECAPACITY (include/str_er.h)
OCR_BIG_PX, OCR_BIG_CAP = 4096, 4095          # ocr_device.h: boxes above BIG_PX pixels are queued, at most BIG_CAP of them
NEAR25 = float(np.nextafter(25.0, 0))
NAN = float("nan")


# ---- records ------------------------------------------------------------------------------------------------------------------
def _er(n, **kw):
    e = np.zeros(n, ER)
    e["w"], e["h"], e["area"], e["cls"] = 20, 30, 400, 2
    e["color1"], e["color2"], e["color3"] = 100.0, 120.0, 130.0
    for k, v in kw.items():
        e[k] = v
    return e


def _finish(e):
    assert e["x"].min(initial=0) >= 0 and e["y"].min(initial=0) >= 0 and e["w"].min(initial=1) >= 1 and e["h"].min(initial=1) >= 1
    assert (e["x"] + e["w"]).max(initial=0) <= 65535 and (e["y"] + e["h"]).max(initial=0) <= 65535        # CAND_DTYPE keeps them in 16 bits
    e["id"] = np.arange(len(e))
    e["cx"], e["cy"] = e["x"] + e["w"] // 2, e["y"] + e["h"] // 2
    return e


def _place(e, i, cx, cy):
    """Put record i so that its centre (x + w / 2, y + h / 2) is (cx, cy)."""
    e[i]["x"], e[i]["y"] = cx - e[i]["w"] // 2, cy - e[i]["h"] // 2


def _cands(S, e):
    cd = np.zeros(len(e), S.CAND_DTYPE)
    for k in ("x", "y", "w", "h", "area", "cls"):
        cd[k] = e[k]
    return cd, np.stack([e["color1"], e["color2"], e["color3"]], axis=1).reshape(-1, 3)


def _tracks(S, e, tracked):
    tr = np.zeros(len(e), S.TRACK_DTYPE)
    for k in ("color1", "color2", "color3", "cx", "cy"):
        tr[k] = e[k]
    tr["tracked"] = tracked
    return tr


# ---- the two rules in numpy (for generations and pair counts; both are checked against the oracle in the CPU section) ------------
def _track_rule_np(s, w):
    sw, sh, ww, wh, sa, wa = (a.astype(np.int64) for a in (s["w"], s["h"], w["w"], w["h"], s["area"], w["area"]))
    with np.errstate(invalid="ignore"):
        return ((np.abs(s["cx"] - w["cx"]) + np.abs(s["cy"] - w["cy"]) < (np.maximum(sw, sh) << 1)) & (np.abs(sh - wh) < np.minimum(sh, wh)) &
                (np.abs(sw - ww) < ((sw + ww) >> 1)) & (np.abs(s["color1"] - w["color1"]) < 25) & (np.abs(s["color2"] - w["color2"]) < 25) &
                (np.abs(s["color3"] - w["color3"]) < 25) & (np.abs(sa - wa) < np.minimum(sa, wa) * 3))


def _group_rule_np(a, b):
    aw, ah, bw, bh, aa, ba = (v.astype(np.int64) for v in (a["w"], a["h"], b["w"], b["h"], a["area"], b["area"]))
    with np.errstate(invalid="ignore"):
        return ((np.abs(a["cx"] - b["cx"]) < np.maximum(aw, bw) * 3.0) & (np.abs(a["cy"] - b["cy"]) < (ah + bh) * 0.25) &
                (np.abs(ah - bh) < np.minimum(ah, bh)) & (np.abs(aw - bw) < np.minimum(ah, bh * 2)) &
                (np.abs(a["color1"] - b["color1"]) < 25) & (np.abs(a["color2"] - b["color2"]) < 25) &
                (np.abs(a["color3"] - b["color3"]) < 25) & (np.abs(aa - ba) < np.minimum(aa, ba) * 4))


def _generations(e):
    """er_track's closure as a breadth-first search: generation of every record (0 strong, -1 not tracked)."""
    e = _finish(e.copy())
    gen = np.where(e["cls"] == 1, 0, -1)
    front, g = np.nonzero(e["cls"] == 1)[0], 0
    while len(front):
        rest = np.nonzero((e["cls"] == 2) & (gen < 0))[0]
        if not len(rest):
            break
        new = rest[_track_rule_np(e[front][:, None], e[rest][None, :]).any(axis=0)]
        g += 1
        gen[new] = g
        front = new
    return gen


def _n_group_pairs(oracle, e):
    """Pairs the grouping rule passes over the sorted list of the (all tracked) records e."""
    s = e[oracle.er_grouping(e)[0]]
    return int(np.triu(_group_rule_np(s[:, None], s[None, :]), 1).sum())


# =================================================================================================================================
# 1. er_track
# =================================================================================================================================
def _pairs(cases, rule):
    """cases: (name, tied, first record's fields, second record's fields, centre offset of the second).  Every pair sits 1500
    pixels from the next one: nothing of one pair is near anything of another.  rule 'track': first strong, second weak."""
    e = _er(2 * len(cases))
    for k, (_, _, a, b, (dx, dy)) in enumerate(cases):
        for i, fields in ((2 * k, a), (2 * k + 1, b)):
            for f, v in fields.items():
                e[i][f] = v
        if rule == "track":
            e[2 * k]["cls"] = 1
        cx, cy = 700 + 1500 * (k % 40), 700 + 1500 * (k // 40)
        _place(e, 2 * k, cx, cy)
        _place(e, 2 * k + 1, cx + dx, cy + dy)
    return _finish(e)


def _colour_cases():
    out = []
    for c in ("color1", "color2", "color3"):
        out += [(c + " == 25", False, {c: 100.0}, {c: 125.0}), (c + " == -25", False, {c: 100.0}, {c: 75.0}),
                (c + " just under 25", True, {c: 0.0}, {c: NEAR25}), (c + " just under -25", True, {c: NEAR25}, {c: 0.0}),
                (c + " 24", True, {c: 100.0}, {c: 124.0}), (c + " 26", False, {c: 100.0}, {c: 126.0}),
                (c + " NaN first", False, {c: NAN}, {c: 100.0}), (c + " NaN second", False, {c: 100.0}, {c: NAN}), (c + " NaN both", False, {c: NAN}, {c: NAN})]
    return out


@functools.lru_cache(None)
def track_clause_cases():
    """track_rule's seven clauses at equality, one unit inside and one unit outside (s: 20 x 30, area 400 unless stated)."""
    near = (10, 0)
    cases = [("centre == 2 max", False, {}, {}, (40, 20)), ("centre inside", True, {}, {}, (40, 19)), ("centre outside", False, {}, {}, (40, 21)),
             ("centre == 2 max, negative", False, {}, {}, (-40, -20)), ("centre inside, negative", True, {}, {}, (-19, -40)),
             ("centre == 2 max(w)", False, {"w": 50}, {"w": 50}, (100, 0)), ("centre inside 2 max(w)", True, {"w": 50}, {"w": 50}, (0, 99)),
             ("dh == min", False, {}, {"h": 60}, near), ("dh inside", True, {}, {"h": 59}, near), ("dh outside", False, {}, {"h": 61}, near),
             ("dh == min, smaller", False, {}, {"h": 15}, near), ("dh inside, smaller", True, {}, {"h": 16}, near), ("dh outside, smaller", False, {}, {"h": 14}, near),
             ("dw 20 == 40 >> 1", False, {"w": 10}, {"w": 30}, near), ("dw 18 < 38 >> 1", True, {"w": 10}, {"w": 28}, near), ("dw 21 > 41 >> 1", False, {"w": 10}, {"w": 31}, near),
             ("dw 19 == 39 >> 1", False, {"w": 10}, {"w": 29}, near),
             ("dw 20 == 40 >> 1, smaller", False, {"w": 30}, {"w": 10}, near), ("dw 19 < 41 >> 1, smaller", True, {"w": 30}, {"w": 11}, near),
             ("dw 19 == 39 >> 1, smaller", False, {"w": 29}, {"w": 10}, near),
             ("da == 3 min", False, {}, {"area": 1600}, near), ("da inside", True, {}, {"area": 1599}, near), ("da outside", False, {}, {"area": 1601}, near),
             ("da == 3 min, smaller", False, {}, {"area": 100}, near), ("da inside, smaller", True, {}, {"area": 101}, near), ("da outside, smaller", False, {}, {"area": 99}, near)]
    cases += [(n, t, a, b, near) for (n, t, a, b) in _colour_cases()]
    return cases, _pairs(cases, "track")


@functools.lru_cache(None)
def track_direction():
    """A (14 x 14) and B (10 x 10) at L1 distance 27: 2 max(B) = 20 <= 27 < 28 = 2 max(A).  Records 0, 1: A strong, B weak; 2, 3: B strong, A weak."""
    e = _er(4, area=100, w=10, h=10)
    for i in (0, 3):
        e[i]["w"], e[i]["h"], e[i]["area"] = 14, 14, 150
    e["cls"] = (1, 2, 1, 2)
    _place(e, 0, 1000, 1000); _place(e, 1, 1025, 1002)
    _place(e, 2, 5025, 1002); _place(e, 3, 5000, 1000)
    return _finish(e)


@functools.lru_cache(None)
def track_chain(G=300):
    """One strong ER and G weak ones in a row, 40 pixels apart (2 max(w, h) = 60): w_k is tied to w_k-1 only.  Shuffled: returns
    the records and pos[i] = place of record i in the chain (= its generation)."""
    e = _er(G + 1, y=1000)
    e["x"] = 100 + 40 * np.arange(G + 1)
    e[0]["cls"] = 1
    pos = np.random.default_rng(1234).permutation(G + 1)
    return _finish(e[pos]), pos


@functools.lru_cache(None)
def track_rings(K=3000):
    """One strong ER (400 x 400), K weak ones tied to it (250 x 250, centres within 700 of its centre), K more (130 x 130) each
    within 400 of one of the first ring: the strong ER's height clause excludes them (270 >= 130).  The rings alternate in
    candidate order, the strong ER sits in the middle."""
    rng = np.random.default_rng(4321)
    e = _er(2 * K + 1, area=40000)
    ring1, ring2 = np.arange(0, 2 * K, 2), np.arange(1, 2 * K, 2)
    ring1[ring1 >= K] += 1; ring2[ring2 >= K] += 1           # index K is the strong ER
    e["w"][K] = e["h"][K] = 400; e["cls"][K] = 1
    e["w"][ring1] = e["h"][ring1] = 250
    e["w"][ring2] = e["h"][ring2] = 130
    c1 = 10200 + rng.integers(-350, 351, (K, 2))
    c2 = c1 + rng.integers(-200, 201, (K, 2))
    _place(e, K, 10200, 10200)
    for idx, c in ((ring1, c1), (ring2, c2)):
        e["x"][idx], e["y"][idx] = c[:, 0] - e["w"][idx] // 2, c[:, 1] - e["h"][idx] // 2
    return _finish(e), ring1, ring2


TRACK_COUNTS = (1, 255, 256, 257, 511, 512, 513, 1500)


@functools.lru_cache(None)
def track_count_case(n):
    """n records: the chain cut to min(301, max(1, 2 n / 3)) members, cls = 0 records ON the chain (they would be tied if they were
    weak) and weak records far from everything, shuffled -- with the chain's last member as the last record."""
    chain, pos = track_chain()
    L = min(len(chain), max(1, 2 * n // 3))
    e = _er(n, y=1000)
    e[:L] = chain[np.argsort(pos)][:L]
    pad = np.arange(L, n)
    e["cls"][pad[0::2]] = 0
    e["x"][pad[0::2]] = 100 + 40 * (np.arange(len(pad[0::2])) % L)
    e["x"][pad[1::2]] = 100 + 90 * np.arange(len(pad[1::2])); e["y"][pad[1::2]] = 3000          # 90 apart: tied to nothing, each other included
    order = np.random.default_rng(n).permutation(n)
    order = np.concatenate([order[order != L - 1], [L - 1]])
    return _finish(e[order]), L


def track_special_cases():
    chain = track_chain()[0]
    no_strong = chain.copy(); no_strong["cls"] = 2
    all_strong = chain.copy(); all_strong["cls"] = 1
    pool_only = chain.copy(); pool_only["cls"] = 0
    return {"empty": _finish(_er(0)), "no strong": _finish(no_strong), "all strong": _finish(all_strong), "only cls 0": _finish(pool_only)}


@functools.lru_cache(None)
def track_random(trial):
    rng = np.random.default_rng(500 + trial)
    n = int(rng.integers(600, 1201))
    e = _er(n)
    e["x"], e["y"] = rng.integers(0, 2400, n), rng.integers(0, 500, n)
    e["w"], e["h"] = rng.integers(4, 40, n), rng.integers(6, 48, n)
    e["area"] = (e["w"].astype(np.int64) * e["h"] * rng.uniform(0.3, 1.0, n)).astype(np.int64) + 1
    e["cls"] = rng.choice([0, 1, 2], n, p=[0.2, 0.01, 0.79])
    for k in ("color1", "color2", "color3"):
        e[k] = rng.integers(100, 125, n) + rng.integers(0, 4, n) * 0.25         # a narrow band: most colour clauses pass
    e["color2"][rng.random(n) < 0.02] = np.nan
    return _finish(e)


def _tracked_set(oracle, e):
    order, out = oracle.er_track(e)
    assert len(set(order.tolist())) == len(order)
    return set(order.tolist()), out


# ---- CPU: the inputs have their properties ---------------------------------------------------------------------------------------
def test_track_clause_cases_sit_on_the_boundaries(oracle):
    cases, e = track_clause_cases()
    names = [c[0] for c in cases]
    for must in ("dw 19 == 39 >> 1", "dw 18 < 38 >> 1", "da == 3 min", "centre == 2 max", "color1 == 25", "color2 just under 25", "color3 NaN second"):
        assert must in names
    assert (10 + 29) >> 1 == 19 and abs(0.0 - NEAR25) < 25 and NEAR25 != 25.0 and 100.0 + NEAR25 == 125.0       # (hence 0.0, not 100.0, on the other side)
    want = {2 * k for k in range(len(cases))} | {2 * k + 1 for k, c in enumerate(cases) if c[1]}
    got, _ = _tracked_set(oracle, e)
    assert got == want, [names[i // 2] for i in sorted(got ^ want)]
    for k, c in enumerate(cases):                                  # a pair alone gives what it gives among the others
        assert _tracked_set(oracle, e[2 * k:2 * k + 2])[0] == ({0, 1} if c[1] else {0}), c[0]
    # exactly one of the three pairs of a clause's triple is tied
    for stem in ("dh", "da"):
        assert [c[1] for c in cases if c[0] in (stem + " == min", stem + " == 3 min", stem + " inside", stem + " outside")] == [False, True, False]


def test_track_direction_is_one_sided(oracle):
    e = track_direction()
    d = abs(int(e[0]["cx"]) - int(e[1]["cx"])) + abs(int(e[0]["cy"]) - int(e[1]["cy"]))
    assert 2 * max(e[1]["w"], e[1]["h"]) <= d < 2 * max(e[0]["w"], e[0]["h"])
    assert d == abs(int(e[2]["cx"]) - int(e[3]["cx"])) + abs(int(e[2]["cy"]) - int(e[3]["cy"]))
    assert _tracked_set(oracle, e)[0] == {0, 1, 2}


def test_track_chain_is_300_generations_deep(oracle):
    e, pos = track_chain()
    G = len(e) - 1
    assert G == 300 and _tracked_set(oracle, e)[0] == set(range(G + 1))
    cut = e[pos != 150]
    assert len(_tracked_set(oracle, cut)[0]) == 150                       # the strong ER and w_1 .. w_149
    gen = _generations(e)
    assert (gen == pos).all() and gen.max() == 300
    assert (np.diff(pos) < 0).sum() > G // 3                               # generation does not follow the candidate index


def test_track_rings_are_wider_than_the_workgroup(oracle):
    e, ring1, ring2 = track_rings()
    K = len(ring1)
    assert K == 3000 and (np.abs(ring1[:100] - ring2[:100]) == 1).all()   # interleaved
    got, _ = _tracked_set(oracle, e)
    assert got == set(range(2 * K + 1))
    keep = np.ones(len(e), bool); keep[ring1] = False
    assert len(_tracked_set(oracle, e[keep])[0]) == 1                       # without the first ring nothing reaches the second
    keep = np.ones(len(e), bool); keep[ring2] = False
    assert len(_tracked_set(oracle, e[keep])[0]) == K + 1                   # the first ring hangs on the strong ER alone
    s = e[K:K + 1]
    assert _track_rule_np(s, e[ring1]).all() and not _track_rule_np(s, e[ring2]).any()


def test_track_count_cases(oracle):
    for n in TRACK_COUNTS:
        e, L = track_count_case(n)
        assert len(e) == n
        got, _ = _tracked_set(oracle, e)
        assert len(got) == L and (n - 1) in got                             # the chain's end is the last record
        if n > 1:
            assert (e["cls"] == 0).sum() > 0 and ((e["cls"] == 2).sum() > L - 1 or n < 4)
        gen = _generations(e)
        assert gen.max() == L - 1 and gen[n - 1] == L - 1
    sp = track_special_cases()
    assert _tracked_set(oracle, sp["empty"])[0] == set() and _tracked_set(oracle, sp["no strong"])[0] == set()
    assert _tracked_set(oracle, sp["only cls 0"])[0] == set() and len(_tracked_set(oracle, sp["all strong"])[0]) == len(sp["all strong"])


def test_track_random_clusters_are_deep_and_bfs_is_the_oracle(oracle):
    deepest = 0
    for trial in range(6):
        e = track_random(trial)
        gen = _generations(e)
        got, _ = _tracked_set(oracle, e)
        assert got == set(np.nonzero(gen >= 0)[0].tolist())                 # the numpy BFS finds the oracle's set
        assert 0 < len(got) < (e["cls"] != 0).sum()
        deepest = max(deepest, int(gen.max()))
    assert deepest >= 3
    assert max(len(track_random(t)) for t in range(6)) > 1024


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _check_track(erf, S, oracle, e):
    cd, cols = _cands(S, e)
    want, out = _tracked_set(oracle, e)
    for _ in range(2):                                                     # the frontier is appended with atomics: its order may differ, the set may not
        tr, cx, cy = erf.er_track(cd, cols)
        assert set(np.nonzero(tr)[0].tolist()) == want
        assert (cx == out["cx"]).all() and (cy == out["cy"]).all()
    return want


@pytest.mark.gpu
def test_gpu_track_clause_boundaries_and_direction(erf, oracle, S):
    """track_rule clause by clause at equality / inside / outside (`>> 1` on an odd sum, 25.0 and the double below it, NaN), and its one-sidedness."""
    _check_track(erf, S, oracle, track_clause_cases()[1])
    assert _check_track(erf, S, oracle, track_direction()) == {0, 1, 2}


@pytest.mark.gpu
def test_gpu_track_deep_chain_and_wide_rings(erf, oracle, S):
    """k_er_track's frontier loop: 300 generations of one member each, then two generations of 3000 members (12 x the workgroup)."""
    assert len(_check_track(erf, S, oracle, track_chain()[0])) == 301
    assert len(_check_track(erf, S, oracle, track_rings()[0])) == 6001


@pytest.mark.gpu
@pytest.mark.parametrize("n", TRACK_COUNTS)
def test_gpu_track_counts(erf, oracle, S, n):
    """Candidate counts around the 256-thread stride, the deepest member of the closure in the last record."""
    e, L = track_count_case(n)
    assert len(_check_track(erf, S, oracle, e)) == L


@pytest.mark.gpu
def test_gpu_track_special_cases(erf, oracle, S):
    """No candidates, no strong ER, only strong ERs, only pool records."""
    for name, e in track_special_cases().items():
        got = _check_track(erf, S, oracle, e)
        assert len(got) == (len(e) if name == "all strong" else 0), name


@pytest.mark.gpu
def test_gpu_track_random_clusters(erf, oracle, S):
    """Dense random clusters of up to 1200 candidates: closures of up to 25 generations."""
    for trial in range(6):
        _check_track(erf, S, oracle, track_random(trial))


# =================================================================================================================================
# 2. er_grouping
# =================================================================================================================================
@functools.lru_cache(None)
def group_clause_cases():
    """group_rule's eight clauses at equality, inside and outside.  The first record of a pair has the smaller centre x unless the
    offset is negative: then the second one comes first in the sorted list and is the rule's `a`."""
    tall = {"h": 40}
    cases = [("dcx == 3 max", False, {}, {}, (60, 0)), ("dcx inside", True, {}, {}, (59, 0)), ("dcx outside", False, {}, {}, (61, 0)),
             ("dcx == 3 max(b.w)", False, tall, {"h": 40, "w": 50}, (150, 0)), ("dcx inside 3 max(b.w)", True, tall, {"h": 40, "w": 50}, (149, 0)),
             ("dcx == 3 max(a.w)", False, {"h": 40, "w": 50}, tall, (150, 0)), ("dcx inside 3 max(a.w)", True, {"h": 40, "w": 50}, tall, (149, 0)),
             ("dcx == 0", True, {}, {}, (0, 3)),
             ("dcy 15 < 61 / 4", True, {}, {"h": 31}, (10, 15)), ("dcy 15 == 60 / 4", False, {}, {}, (10, 15)), ("dcy 14 < 60 / 4", True, {}, {}, (10, 14)),
             ("dcy 16 > 60 / 4", False, {}, {}, (10, 16)), ("dcy -15 < 61 / 4", True, {"h": 31}, {}, (10, -15)), ("dcy -15 == 60 / 4", False, {}, {}, (10, -15)),
             ("dcy 15 < 62 / 4", True, {"h": 31}, {"h": 31}, (10, 15)), ("dcy 16 > 62 / 4", False, {"h": 31}, {"h": 31}, (10, 16)),
             ("dcy 15 < 63 / 4", True, {"h": 31}, {"h": 32}, (10, 15)), ("dcy 16 > 63 / 4", False, {"h": 31}, {"h": 32}, (10, 16)),
             ("dh == min", False, {}, {"h": 60}, (10, 0)), ("dh inside", True, {}, {"h": 59}, (10, 0)), ("dh outside", False, {}, {"h": 61}, (10, 0)),
             ("dw 30 < min(40, 42)", True, {"h": 40}, {"h": 21, "w": 50}, (30, 0)), ("dw 30 >= min(21, 80)", False, {"h": 40}, {"h": 21, "w": 50}, (-30, 0)),
             ("dw == min(a.h, 2 b.h)", False, tall, {"w": 60}, (30, 0)), ("dw inside", True, tall, {"w": 59}, (30, 0)), ("dw outside", False, tall, {"w": 61}, (30, 0)),
             ("da == 4 min", False, {}, {"area": 2000}, (10, 0)), ("da inside", True, {}, {"area": 1999}, (10, 0)), ("da outside", False, {}, {"area": 2001}, (10, 0)),
             ("da == 4 min, smaller", False, {}, {"area": 80}, (10, 0)), ("da inside, smaller", True, {}, {"area": 81}, (10, 0))]
    cases += [(n, t, a, b, (10, 0)) for (n, t, a, b) in _colour_cases()]
    e = _pairs(cases, "group")
    e["cls"] = 1
    return cases, e


@functools.lru_cache(None)
def inner_sup_cases():
    """(container, contained) pairs 2000 pixels apart; sup[k]: the contained box of pair k goes."""
    cases = [("centre distance == 0.2 * 50", False, (50, 50), (20, 20), (21, 23)),           # centre offsets (6, 8): distance 10.0
             ("centre distance sqrt(85)", True, (50, 50), (20, 20), (21, 22)),                # (6, 7)
             ("centre distance == 0.2 * 50, axis", False, (50, 50), (20, 20), (25, 15)),      # (10, 0)
             ("centre distance 9", True, (50, 50), (20, 20), (24, 15)),
             ("max(w, h) takes w", False, (50, 20), (10, 8), (30, 6)),                         # (10, 0) of a 50 x 20 box
             ("max(w, h) takes h", False, (20, 50), (8, 10), (6, 30)),
             ("area ratio == 2", False, (50, 50), (25, 50), (12, 0)), ("area ratio 2500 / 1225", True, (50, 50), (25, 49), (12, 0)),
             ("equal left and top edges", True, (100, 20), (80, 12), (0, 0)), ("equal right and bottom edges", True, (100, 20), (80, 12), (20, 8)),
             ("one pixel over the right edge", False, (100, 20), (80, 12), (21, 8)), ("one pixel over the bottom edge", False, (100, 20), (80, 12), (20, 9)),
             ("the same box twice", False, (50, 50), (50, 50), (0, 0))]
    e = _er(2 * len(cases), cls=1)
    for k, (_, _, (aw, ah), (bw, bh), (ox, oy)) in enumerate(cases):
        x, y = 500 + 2000 * (k % 30), 500 + 2000 * (k // 30)
        e[2 * k]["x"], e[2 * k]["y"], e[2 * k]["w"], e[2 * k]["h"] = x, y, aw, ah
        e[2 * k + 1]["x"], e[2 * k + 1]["y"], e[2 * k + 1]["w"], e[2 * k + 1]["h"] = x + ox, y + oy, bw, bh
    return cases, _finish(e)


GROUP_NT = (255, 256, 257, 511, 512, 513, 1025)
N_CX = 40


@functools.lru_cache(None)
def group_chunk_case(n_t):
    """n_t tracked records among untracked ones, centre x from 40 values 5 apart (equal keys in every chunk of the sorted list and
    across its chunk boundaries).  Returns (records, tracked flags, notes).  Planted, all tracked:
      * C1 (first record, centre x = the smallest value) contains X (last record, centre x = the largest value) contains D
        (second record, the smallest value): container and contained at the two ends of the sorted list, in both orders;
      * a 600 x 600 box around 30 small ones with the six smallest centre x values: 30 suppressed boxes early in the sorted list,
        so the kept count passes 256 later than the position does."""
    rng = np.random.default_rng(9000 + n_t)
    n_un = 300 + n_t // 3
    n = n_t + n_un
    val = 3000 + 5 * np.arange(N_CX)
    e = _er(n, cls=1)
    e["w"], e["h"] = rng.integers(4, 40, n), rng.integers(6, 48, n)
    e["area"] = (e["w"].astype(np.int64) * e["h"] * rng.uniform(0.3, 1.0, n)).astype(np.int64) + 1
    e["x"] = val[rng.integers(0, N_CX, n)] - e["w"] // 2
    e["y"] = rng.integers(0, 6000, n)
    for k in ("color1", "color2", "color3"):
        e[k] = rng.integers(95, 125, n)
    e["color3"][rng.random(n) < 0.02] = np.nan
    tracked = np.zeros(n, bool)
    tracked[rng.permutation(n - 2)[:n_t - 2] + 1] = True                    # (records 0 and n - 1 are planted below)
    tracked[[0, n - 1]] = True
    t_idx = np.nonzero(tracked)[0]
    assert len(t_idx) == n_t
    # the chain C1 > X > D
    d = int(t_idx[1])
    for i, (w, h, cx) in ((0, (2400, 300, val[0])), (n - 1, (1100, 100, val[-1])), (d, (20, 20, val[0]))):
        e[i]["w"], e[i]["h"], e[i]["area"] = w, h, w * h // 2
        _place(e, i, int(cx), 30150)
    # the nest: record t_idx[2] holds t_idx[3 .. 32]
    nest = t_idx[2:33]
    e["w"][nest[0]], e["h"][nest[0]], e["area"][nest[0]] = 600, 600, 100000
    _place(e, int(nest[0]), int(val[2]), 40300)
    for j, i in enumerate(nest[1:]):
        e[i]["w"], e[i]["h"], e[i]["area"] = 10, 10, 60
        _place(e, int(i), int(val[j % 6]), 40300 - 45 + 3 * j)
    return _finish(e), tracked, {"c1": 0, "x": n - 1, "d": d, "nest": nest}


@functools.lru_cache(None)
def group_growth_case():
    """Eight clusters of 60 near-identical boxes, 2000 pixels apart: every pair of a cluster passes, none across clusters."""
    rng = np.random.default_rng(60)
    e = _er(480, cls=1)
    k = np.arange(480)
    e["x"] = 1000 + 2000 * (k % 8) + rng.integers(0, 3, 480)
    e["y"] = 1000 + rng.integers(0, 3, 480)
    return _finish(e)


def _first_pair_capacity(n):
    """group_phase asks for max(8 n, 4096) entries and gets a quarter more (ensure_quarter_more)."""
    need = max(8 * n, 4096)
    return need + need // 4


def _ref_all(oracle, e, tracked, inner, overlap=False):
    """The oracle's all_er (record indices) for the tracked records of e."""
    keep = np.nonzero(tracked)[0]
    return keep[oracle.er_grouping(e[keep], overlap_sup=overlap, inner_sup=inner)[0]]


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_group_clause_cases_sit_on_the_boundaries(oracle):
    cases, e = group_clause_cases()
    names = [c[0] for c in cases]
    for must in ("dcy 15 < 61 / 4", "dcy 15 == 60 / 4", "dw 30 < min(40, 42)", "dw 30 >= min(21, 80)", "dcx == 3 max", "da == 4 min"):
        assert must in names
    _, lines, _ = oracle.er_grouping(e)
    got = {frozenset(int(m) for m in l[0]) for l in lines}
    want = {frozenset((2 * k, 2 * k + 1)) for k, c in enumerate(cases) if c[1]}
    assert got == want, [names[min(s) // 2] for s in got ^ want]
    assert all(len(l[0]) == 2 for l in lines)
    k = names.index("dw 30 >= min(21, 80)")
    assert e[2 * k + 1]["cx"] < e[2 * k]["cx"] and e[2 * k + 1]["h"] == 21            # the 21-high box comes first there
    assert _n_group_pairs(oracle, e) == len(want)


def test_inner_sup_cases_sit_on_the_boundaries(oracle):
    cases, e = inner_sup_cases()
    gone = {2 * k + 1 for k, c in enumerate(cases) if c[1]}
    assert set(oracle.er_grouping(e, inner_sup=True)[0].tolist()) == set(range(len(e))) - gone
    assert len(oracle.er_grouping(e, inner_sup=False)[0]) == len(e)
    a, b = e[0], e[1]
    assert (a["cx"] - b["cx"]) ** 2 + (a["cy"] - b["cy"]) ** 2 == 100 and max(a["w"], a["h"]) == 50


def test_group_chunk_cases_straddle_the_chunks(oracle):
    kept_late = 0
    for n_t in GROUP_NT:
        e, tracked, note = group_chunk_case(n_t)
        assert tracked.sum() == n_t and len(e) // 256 > n_t // 256                       # untracked records push the tracked ones over more chunk edges
        plain = _ref_all(oracle, e, tracked, False)
        assert len(plain) == n_t and len(np.unique(e["cx"][tracked])) <= N_CX + 1
        pos = {int(r): p for p, r in enumerate(plain)}
        cx = e["cx"][plain]
        for edge in range(256, n_t, 256):                                                # equal keys across every chunk edge of the sorted list
            assert cx[edge - 1] == cx[edge], (n_t, edge)
        assert pos[note["c1"]] == 0 and pos[note["d"]] == 1 and pos[note["x"]] == n_t - 1
        sup = _ref_all(oracle, e, tracked, True)
        gone = set(plain.tolist()) - set(sup.tolist())
        assert {note["x"], note["d"]} <= gone and set(note["nest"][1:].tolist()) <= gone and note["c1"] not in gone
        if n_t > 256:
            # container first (C1 at 0, X in the last chunk) and contained first (D at 1, its only container besides C1 ... X in the last chunk)
            assert pos[note["x"]] // 256 > 0 == pos[note["c1"]] // 256 == pos[note["d"]] // 256
            only_x = e[[note["x"], note["d"]]].copy()
            assert set(oracle.er_grouping(only_x, inner_sup=True)[0].tolist()) == {0}    # X alone removes D
        kept_mask = np.array([int(r) not in gone for r in plain])
        if n_t >= 511:
            assert kept_mask[:256].sum() < 256 - 25 and kept_mask.sum() > 256            # the kept count crosses 256 in a later chunk than the position
            kept_late += 1
        for inner in (False, True):
            assert len(_ref_all(oracle, e, tracked, inner, overlap=True)) <= len(_ref_all(oracle, e, tracked, inner))
        assert len(oracle.er_grouping(e[tracked], inner_sup=True)[1]) > 3                # and there are lines to compare
    assert kept_late == 4


def test_group_growth_case_overflows_the_first_pair_buffer(oracle):
    e = group_growth_case()
    n_pairs = _n_group_pairs(oracle, e)
    assert n_pairs == 8 * 1770 and n_pairs > 2 * _first_pair_capacity(len(e))
    _, lines, _ = oracle.er_grouping(e)
    assert len(lines) == 8 and all(len(l[0]) == 1771 for l in lines)                     # a member per pair (and two for the first)
    small = group_clause_cases()[1]
    assert _n_group_pairs(oracle, small) < _first_pair_capacity(len(small)) // 2


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _check_group(f, S, oracle, e, tracked, inner, overlap=False):
    cd, _ = _cands(S, e)
    tr = _tracks(S, e, tracked)
    res = f.er_grouping(cd, tr, overlap_sup=overlap, inner_sup=inner)
    res.cands, res.tracks = cd, tr
    return _check_lines(res, [np.arange(len(e))], oracle, inner, overlap), res


@pytest.mark.gpu
def test_gpu_group_clause_and_inner_sup_boundaries(erf, oracle, S):
    """group_rule clause by clause (the double `* 0.25` and `* 3.0`, min(a.h, 2 b.h) in both sorted orders) and inner_suppression's three conditions at equality."""
    cases, e = group_clause_cases()
    n_lines, res = _check_group(erf, S, oracle, e, True, False)
    assert n_lines == sum(c[1] for c in cases)
    _check_group(erf, S, oracle, e, True, True)
    cases, e = inner_sup_cases()
    gone = {2 * k + 1 for k, c in enumerate(cases) if c[1]}
    _, res = _check_group(erf, S, oracle, e, True, True)
    assert set(res.group_all.tolist()) == set(range(len(e))) - gone
    _, res = _check_group(erf, S, oracle, e, True, False)
    assert len(res.group_all) == len(e)


@pytest.mark.gpu
@pytest.mark.parametrize("n_t", GROUP_NT)
def test_gpu_group_chunk_edges(erf, oracle, S, n_t):
    """k_group_prepare's three chunked loops: the compaction carry, ranks of equal keys across chunk edges, the kept-count carry."""
    e, tracked, _ = group_chunk_case(n_t)
    for inner, overlap in ((False, False), (True, False), (False, True), (True, True)):
        n_lines, res = _check_group(erf, S, oracle, e, tracked, inner, overlap)
        assert n_lines > 3
        assert list(res.group_all) == list(_ref_all(oracle, e, tracked, inner, overlap))


@pytest.mark.gpu
def test_gpu_group_pair_list_growth(oracle, S):
    """group_phase's grow-and-refill: 14160 pairs against a first buffer of 5120 entries, as a context's first call and after a small one.
    (workspace_bytes() does not cover the pair list -- it is an on-demand buffer -- so the growth itself is pinned by the arithmetic above.)"""
    big, small = group_growth_case(), group_clause_cases()[1]
    assert _n_group_pairs(oracle, big) > 2 * _first_pair_capacity(len(big))
    for order in ((big, small, big), (small, big)):
        f = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))       # a fresh context: its pair list starts empty
        for e in order:
            n_lines, res = _check_group(f, S, oracle, e, True, False)
            assert n_lines == (8 if e is big else len(res.texts)) and n_lines > 0
            if e is big:
                assert len(res.text_ers) == 8 * 1771
        f.close()


@pytest.mark.gpu
def test_gpu_group_capacity_refusal(erf, oracle, S):
    """65536 candidates in one image are refused before any launch; 65535 pass; the context stays usable."""
    e = _er(65536, cls=1)
    e["x"] = np.arange(65536) % 60000
    e = _finish(e)
    cd, _ = _cands(S, e)
    tr = _tracks(S, e, False)
    with pytest.raises(S.StrErError) as err:
        erf.er_grouping(cd, tr)
    assert err.value.code == ECAPACITY and "65535" in str(err.value)
    res = erf.er_grouping(cd[:65535], tr[:65535])
    assert len(res.texts) == 0 and len(res.text_ers) == 0 and len(res.group_all) == 0 and len(res.group_bounds) == 65535
    assert (res.group_bounds["x"] == e["x"][:65535]).all() and (res.group_bounds["cx"] == e["cx"][:65535]).all()
    cases, small = group_clause_cases()
    assert _check_group(erf, S, oracle, small, True, False)[0] == sum(c[1] for c in cases)


# =================================================================================================================================
# 3. more than 1024 images in one call
# =================================================================================================================================
N_CROPS, CROP_W, CROP_H = 1040, 160, 96


def crop_frames(S, which=None):
    """Seeded 160 x 96 crops of four 640 x 480 S-text canvases; `which`: only these frames (the same ones the full list has)."""
    rng = np.random.default_rng(2036)
    xy = np.stack([rng.integers(0, 640 - CROP_W + 1, N_CROPS), rng.integers(0, 480 - CROP_H + 1, N_CROPS)], axis=1)
    canvas = {}
    out = []
    for i in (range(N_CROPS) if which is None else which):
        c = i % 4
        if c not in canvas:
            canvas[c] = S.synth.stext_bgr(S.synth.frame_seed(300 + c), 640, 480)
        x, y = int(xy[i, 0]), int(xy[i, 1])
        out.append(np.ascontiguousarray(canvas[c][y:y + CROP_H, x:x + CROP_W]))
    return out


def _oracle_image(oracle, cascades, bgr):
    """The whole reference pipeline on one frame (6 planes, one level): (candidates, tracked, lines)."""
    planes = _ycrcb(oracle, bgr)
    col = np.ascontiguousarray(np.stack([planes[0], planes[1], planes[2]], axis=-1))
    rows = []
    for ch in range(6):
        ref = oracle.detect_plane(planes[ch], cascades[0], cascades[1])
        nodes = ref["tree"].nodes
        for j in np.argsort([int(nodes[i]["key"]) for i in ref["pool"]], kind="stable"):
            nd = nodes[ref["pool"][j]]
            r = _er(1, x=nd["x"], y=nd["y"], w=nd["w"], h=nd["h"], area=nd["area"], cls=ref["cls"][j], ch=ch)
            if r["cls"][0]:
                r["color1"], r["color2"], r["color3"] = oracle.calc_color(planes[ch], col, (nd["x"], nd["y"], nd["w"], nd["h"]))
            rows.append(r)
    e = np.concatenate(rows) if rows else _er(0)
    order, e = oracle.er_track(e)
    return e, order, oracle.er_grouping(e[np.sort(order)])[1]


# the frames the GPU test's assertions rest on (found by running _oracle_image over all 1040 crops)
CROPS_WITH_LINES_LOW, CROPS_WITH_LINES_HIGH, CROP_WITHOUT_TRACKS = (44, 45, 47), (1027, 1030, 1036), 1001


def test_crops_have_lines_on_both_sides_of_1024(S, oracle, oracle_cascades):
    lo, hi, blank = CROPS_WITH_LINES_LOW, CROPS_WITH_LINES_HIGH, CROP_WITHOUT_TRACKS
    assert len(lo) >= 3 and len(hi) >= 3 and max(lo) < 1024 <= min(hi) and min(lo) < blank < max(hi) and max(hi) < N_CROPS
    frames = crop_frames(S, list(lo) + list(hi) + [blank])
    assert all(f.shape == (CROP_H, CROP_W, 3) for f in frames)
    for f in frames[:-1]:
        assert len(_oracle_image(oracle, oracle_cascades, f)[2]) >= 1
    assert len(_oracle_image(oracle, oracle_cascades, frames[-1])[1]) == 0


@pytest.mark.gpu
def test_gpu_track_and_group_on_1040_images(S, cascade_paths, oracle):
    """One call with more images than k_pair_prefix scans in one chunk (1024); k_group_ranges and k_er_track with that many groups."""
    frames = crop_frames(S)
    f = S.ERFilter(params=S.Params(max_width=CROP_W, max_height=CROP_H, max_frames=N_CROPS, n_pyr_levels=1, channel_mask=0x3F))
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    res = f.text_detect_list(frames, S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP)
    f.close()
    planes = {(i, 0): _ycrcb(oracle, frames[i]) for i in range(N_CROPS)}
    order_of_frame = np.argsort(res.cands["frame"], kind="stable")
    assert (order_of_frame == np.arange(len(res.cands))).all()              # candidates come frame by frame
    bounds = np.searchsorted(res.cands["frame"], np.arange(N_CROPS + 1))
    groups, n_tracked = [], []
    # (_expected_tracks selects an image's candidates by a mask over the whole table: it gets one image's slice at a time)
    for i in range(N_CROPS):
        sel = np.arange(bounds[i], bounds[i + 1])
        groups.append(sel)
        if len(sel) == 0:
            n_tracked.append(0)
            continue
        (_, order, e), = _expected_tracks(oracle, types.SimpleNamespace(cands=res.cands[sel]), {(i, 0): planes[(i, 0)]})
        t = res.tracks[sel]
        live = e["cls"] != 0
        for k in ("color1", "color2", "color3"):
            assert np.array_equal(t[k][live], e[k][live], equal_nan=True), i
        assert (t["cx"][live] == e["cx"][live]).all() and (t["cy"][live] == e["cy"][live]).all()
        want = np.zeros(len(sel), bool)
        want[order] = True
        assert (t["tracked"].astype(bool) == want).all(), i
        n_tracked.append(int(want.sum()))
    _check_lines(res, groups, oracle, False)
    with_lines = np.unique(res.texts["frame"])                               # (equal to the oracle's: _check_lines compared every line)
    lo, hi = with_lines[with_lines < 1024], with_lines[with_lines >= 1024]
    assert len(lo) >= 3 and len(hi) >= 3
    assert set(CROPS_WITH_LINES_LOW) <= set(lo.tolist()) and set(CROPS_WITH_LINES_HIGH) <= set(hi.tolist())
    assert any(n_tracked[i] == 0 for i in range(int(lo.min()) + 1, int(hi.max())))
    assert n_tracked[CROP_WITHOUT_TRACKS] == 0


# =================================================================================================================================
# 4. calc_color
# =================================================================================================================================
FW, FH = 640, 360
WIDTHS = (1, 2, 3, 21, 32, 33, 63, 64, 65, 128, 255, 256, 257, 511, 512, 513, 640)
HEIGHTS = (1, 2, 3, 4, 5, 7, 8, 9, 64, 65, 360)


@functools.lru_cache(None)
def color_form_boxes():
    sizes = [(w, h) for w in WIDTHS for h in HEIGHTS] + [(64, 64), (128, 32), (241, 17), (65, 63)]
    boxes = []
    for w, h in sizes:
        for x, y in ((0, 0), (FW - w, 0), (0, FH - h), (FW - w, FH - h)):
            if (x, y, w, h) not in boxes:
                boxes.append((x, y, w, h))
    return np.array(boxes, np.int32)


@functools.lru_cache(None)
def color_big_boxes(n=4200):
    rng = np.random.default_rng(65)
    b = np.empty((n, 4), np.int32)
    b[:, 0], b[:, 1], b[:, 2], b[:, 3] = rng.integers(0, FW - 65 + 1, n), rng.integers(0, FH - 64 + 1, n), 65, 64
    return b


@functools.lru_cache(None)
def color_many_boxes(n=9000):
    """More boxes than one round of resident waves takes on an MI355X (k_ocr_hist: 5 x 256 workgroups of 4 waves = 5120 boxes,
    k_color_sums: 8 x 256 x 4 = 8192): the grid-stride loops run a second round.  Small boxes of all forms, every other one 65 x 64: the
    queue is full before the second round begins."""
    rng = np.random.default_rng(66)
    b = np.empty((n, 4), np.int32)
    b[:, 2], b[:, 3] = rng.integers(1, 40, n), rng.integers(1, 24, n)
    b[::2, 2], b[::2, 3] = 65, 64
    b[:, 0], b[:, 1] = rng.integers(0, FW - b[:, 2] + 1), rng.integers(0, FH - b[:, 3] + 1)
    return b


def old_test_boxes():
    """The 122 boxes of test_gpu_calc_color_matches_oracle (320 x 240)."""
    rng = np.random.default_rng(9)
    boxes = []
    for _ in range(120):
        bw, bh = int(rng.integers(1, 200)), int(rng.integers(1, 160))
        boxes.append((int(rng.integers(0, 320 - bw + 1)), int(rng.integers(0, 240 - bh + 1)), bw, bh))
    return np.array(boxes + [(0, 0, 320, 240), (319, 239, 1, 1)], np.int32)


def _frame_planes(S, oracle, seed, w, h):
    planes = _ycrcb(oracle, S.synth.stext_bgr(S.synth.frame_seed(seed), w, h))
    return planes, np.ascontiguousarray(np.stack([planes[0], planes[1], planes[2]], axis=-1))


def blank_mask_case(S, oracle):
    """A channel with a 300 x 100 block of 255: Otsu on 255 - roi = 0 leaves nothing above the threshold in a box inside the block."""
    planes, col = _frame_planes(S, oracle, 5, FW, FH)
    mask = planes[0].copy()
    mask[50:150, 100:400] = 255
    boxes = np.array([(100, 50, 300, 100), (100, 50, 1, 1), (120, 60, 64, 64), (120, 60, 65, 64), (399, 149, 1, 1), (130, 70, 257, 3), (150, 50, 21, 100),
                      (99, 50, 300, 100), (100, 50, 301, 100)], np.int32)
    return mask, col, boxes, 7            # the first 7 lie inside the block


def test_color_form_boxes_cover_the_forms():
    b = color_form_boxes()
    assert (b[:, 0] >= 0).all() and (b[:, 1] >= 0).all() and (b[:, 0] + b[:, 2] <= FW).all() and (b[:, 1] + b[:, 3] <= FH).all()
    assert set(b[:, 2].tolist()) >= set(WIDTHS) and set(b[:, 3].tolist()) >= set(HEIGHTS)
    px = (b[:, 2] * b[:, 3]).tolist()
    for want in (OCR_BIG_PX - 1, OCR_BIG_PX, OCR_BIG_PX + 1):
        assert want in px
    assert {(64, 64), (128, 32), (241, 17), (65, 63)} <= {(int(w), int(h)) for w, h in b[:, 2:]}
    for w, h in {(int(w), int(h)) for w, h in b[:, 2:]}:
        at = {(int(x), int(y)) for x, y, ww, hh in b if (ww, hh) == (w, h)}
        assert at == {(0, 0), (FW - w, 0), (0, FH - h), (FW - w, FH - h)}
    w = b[:, 2]
    assert ((w <= 64) & (64 % w == 0)).any() and ((w <= 64) & (64 % w != 0)).any() and ((w > 64) & (w <= 256)).any() and (w > 256).any()
    rpp = 64 // np.minimum(w, 64)
    assert ((w <= 64) & (b[:, 3] < 4 * rpp)).any() and ((w <= 64) & (b[:, 3] > 4 * rpp)).any()     # fewer rows than a pass covers, and more
    big = color_big_boxes()
    assert len(big) == 4200 > OCR_BIG_CAP + 1 and (big[:, 2] * big[:, 3] > OCR_BIG_PX).all()
    assert (big[:, 0] + 65 <= FW).all() and (big[:, 1] + 64 <= FH).all() and len(old_test_boxes()) == 122
    many = color_many_boxes()
    assert len(many) > 8 * 256 * 4 and (many[:, 0] + many[:, 2] <= FW).all() and (many[:, 1] + many[:, 3] <= FH).all()
    px = many[:, 2] * many[:, 3]
    assert (px[8192:] > OCR_BIG_PX).sum() > 100 and (px[8192:] <= OCR_BIG_PX).sum() > 100 and (px[:5120] > OCR_BIG_PX).sum() < OCR_BIG_CAP < (px[:8192] > OCR_BIG_PX).sum()
    assert (b[:, 2] <= 300).sum() > 300                                    # enough forms fit a colour image narrower than the mask plane


def test_blank_mask_gives_nan_on_the_oracle(S, oracle):
    mask, col, boxes, n_in = blank_mask_case(S, oracle)
    for k, b in enumerate(boxes):
        c = oracle.calc_color(mask, col, b)
        assert np.isnan(c).all() == (k < n_in), (k, c)
    assert (boxes[:, 2] * boxes[:, 3] > OCR_BIG_PX).any() and (boxes[:n_in, 2] * boxes[:n_in, 3] <= OCR_BIG_PX).any()


def _check_colors(erf, oracle, mask, col, boxes, exp=None):
    got = erf.calc_color(mask, col, boxes)
    if exp is None:
        exp = np.stack([oracle.calc_color(mask, col, b) for b in boxes])
    bad = [k for k in range(len(boxes)) if not np.array_equal(got[k], exp[k], equal_nan=True)]
    assert not bad, [(boxes[k].tolist(), got[k], exp[k]) for k in bad[:5]]
    return exp


@pytest.mark.gpu
def test_gpu_calc_color_box_forms(erf, oracle, S):
    """Every width / height form of color_rows and k_ocr_hist at the frame's four corners, 4095 / 4096 / 4097 pixels, and boxes with an empty Otsu mask (NaN)."""
    planes, col = _frame_planes(S, oracle, 5, FW, FH)
    for mask in (planes[0], planes[4], np.full((FH, FW), 255, np.uint8)):
        _check_colors(erf, oracle, mask, col, color_form_boxes())
    # a colour image smaller than the mask plane (its own stride): it is read from ITS row 0 / column 0 whatever the box's place
    b = color_form_boxes()
    small = b[(b[:, 2] <= 300) & (b[:, 3] <= 200)]
    _check_colors(erf, oracle, planes[4], np.ascontiguousarray(col[:200, :300]), small)
    mask, col, boxes, n_in = blank_mask_case(S, oracle)
    exp = _check_colors(erf, oracle, mask, col, boxes)
    assert np.isnan(exp[:n_in]).all() and not np.isnan(exp[n_in:]).any()


@pytest.mark.gpu
def test_gpu_calc_color_full_big_box_queue(erf, oracle, S):
    """More queued-size boxes than the queue holds: the overflow falls back to the one-wave path in k_ocr_hist and k_color_sums."""
    planes, col = _frame_planes(S, oracle, 5, FW, FH)
    boxes = color_big_boxes()
    exp = _check_colors(erf, oracle, planes[0], col, boxes)                 # 4200 queued-size boxes: 105 of them find the queue full
    for n in (OCR_BIG_CAP, OCR_BIG_CAP + 1):
        _check_colors(erf, oracle, planes[0], col, boxes[:n], exp[:n])
    _check_colors(erf, oracle, planes[0], col, color_many_boxes())          # a second round of the grid-stride loops, the queue full by then
    planes, col = _frame_planes(S, oracle, 2, 320, 240)
    _check_colors(erf, oracle, planes[0], col, old_test_boxes())            # and the context is as good as before
