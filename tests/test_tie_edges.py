"""The sibling-tie passes of a batch at their own limits: what settles sibling_order = 0 behind the first k_nms pass (csrc/er_nms.inl, resolve_sibling_ties in
csrc/str_er_api.cpp).  The planes are tests/tie_planes.py's.

  plane family / batch                                 the line it reaches, from which side
  63 | 64 | 65 | 81 settled planes                     k_alt_list: NMS_ALT_CAP = 64 entries -- below, full, one plane and TIE_SLOTS + 1 planes left over (these
                                                       keep their tie and are walked; in host mode the 17th goes through k_export_listed_planes)
  64 settled + 3 two-glyph planes                      the walked ones (two ties: not for the list) beside a full list; 61 settled + 3 one-glyph walked
                                                       planes: a full list of which the opposite-rule pass must leave three unsettled
  15 | 16 | 17 | 40 walked planes of six sizes         k_tie_slots / k_export_tie_planes: TIE_SLOTS = 16 slots -- below, full, one and 24 planes for
                                                       k_export_listed_planes and the arena of resolve_sibling_ties (hoff, pad_, slot_of); widths 48 | 52 | 51:
                                                       the 16-byte, 4-byte and byte copy of export_plane; the same planes in device memory at an odd pitch
  grids of 127 / 128 / 129 glyphs, a third stroke      the watch list: NMS_WATCH_CAP = 256 -- 254, 255, 256 (sparse: stamps per watched key) and 257, 258 (dense: a
                                                       stamp per pixel) in flood_order_host and in k_flood_order, alone and between sparse planes
  20 dense planes between 20 sparse ones               the arena behind a dense stamp area whose w * h is not a multiple of 64 (the comment at "every term a multiple
                                                       of 256"), at least four dense planes without a slot
  relevance planes at OVERLAP_COEF 0.7                 rel_area in k_nms: area(P) x coef below, one pixel column below, exactly at and above 0.64 rows x cols
  free, kept, noise, rect, changed, noise, settled     k_cand_reprefix / k_cand_move: pools that shrink and grow by a few records between planes whose records move
  1025 planes of 32 x 32                               the second turn of the scans of k_cand_prefix / k_cand_reprefix (carry across 1024 planes) and of the strided
                                                       loops of k_alt_list / k_tie_slots
  15 planes, 40 planes, a dense plane, and again       arena and scratch grow and are reused

The CPU half proves on the oracle alone -- its NMS under the three sibling rules and the census of tie_planes.py -- that every plane has the property it
was made for.  The GPU half compares every plane with the oracle at sibling_mode 0 (node table, pool, classes, scores: `==`) and the growth of
tie_stats()["planes_walked"] with the count derived from NMS_ALT_CAP, TIE_SLOTS and the batch: a plane whose tie the opposite-rule pass settled, or
whose ties are all irrelevant, is not walked.  STR_ER_REPLAY=host and =gpu; where both run, their results are equal byte for byte.

A note on "below" in the relevance family.  A chain that competes for P starts at a node whose box exceeds coef x area(P); the pool takes only boxes with
w < 0.8 cols and h < 0.8 rows.  On 50 x 70 the largest such box is 56 x 39 = 2184 (cols * 0.8 is 56.00000000000001 in doubles, in k_nms and in the oracle)
< 2240 = 0.64 x 3500: with integer boxes the pools can differ only where area(P) x coef < 2184.  So there are two planes below: one far enough below
that the pools of the rules differ ("differs"), and one a single pixel column below ("just below"), where the rule is on the safe side -- the plane is
walked although no order changes its pool.

Not reached: a context with fewer than 16 slots (the clamp to 4 needs planes of 16 MB); the 1 GB round limit of the replay scratch (as many pixels
in tie planes of one batch); `fits == false` in k_tie_slots (no public call puts a plane larger than max_width x max_height into a batch).
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import tie_planes as tp
from conftest import check_plane_against_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scene-text-recognition_amd", "csrc")


def _constant(header, name):
    """`constexpr int NAME = value;` as the header states it."""
    with open(os.path.join(CSRC, header)) as fh:
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, fh.read())
    assert m, "%s not found in %s" % (name, header)
    return int(m.group(1))


ALT_CAP = _constant("er_types.h", "NMS_ALT_CAP")
WATCH_CAP = _constant("er_types.h", "NMS_WATCH_CAP")
TIE_SLOTS = _constant("str_er_ctx.h", "TIE_SLOTS")
CHUNK = 1024                               # planes per turn of the scan loops of k_cand_prefix / k_cand_reprefix (their workgroup)


# =================================================================================================================================
# the planes and the batches
# =================================================================================================================================
@functools.lru_cache(None)
def two_glyph_plane():
    """48 x 48 with two transposed glyphs on its diagonal: two ties, so not a plane for the opposite-rule pass; walked, and neither key rule gives its pool."""
    t, p = tp.flipped(tp.glyph_plane(24, 24, 20, 20, 2, 2), "T"), tp.free_plane(48, 48)
    p[:24, :24] = p[24:, 24:] = t
    return p


@functools.lru_cache(None)
def alt_batch(n_settled, walked=""):
    """(planes, kinds): n_settled settled planes of 48 x 48 (every second one transposed), a tie-free plane behind every third, and the walked planes
    ('two': two_glyph_plane, 'one': kept / changed) at the start, in the middle and at the end."""
    extra = {"": [], "two": [two_glyph_plane()] * 3, "one": [tp.kept_plane(), tp.changed_plane(), tp.flipped(tp.kept_plane(), "r180")]}[walked]
    planes, kinds = [], []
    for k in range(n_settled):
        if extra and k in (0, n_settled // 2):
            planes.append(extra[len([x for x in kinds if x == "walked"])]); kinds.append("walked")
        planes.append(tp.settled_plane(transposed=bool(k % 2))); kinds.append("settled")
        if k % 3 == 2:
            planes.append(tp.rect_plane(48, 48, 3 + k % 20, 5 + k % 17, 14, 12) if k % 2 else tp.free_plane(48, 48)); kinds.append("free")
    if extra:
        planes.append(extra[2]); kinds.append("walked")
    return planes, kinds


ALT_CASES = {"63": (ALT_CAP - 1, "", 0), "64": (ALT_CAP, "", 0), "65": (ALT_CAP + 1, "", 1), "81": (ALT_CAP + TIE_SLOTS + 1, "", TIE_SLOTS + 1),
             "64 + 3 walked": (ALT_CAP, "two", 3), "61 + 3 of one tie": (ALT_CAP - 3, "one", 3)}           # name -> (settled, walked kind, planes walked)


@functools.lru_cache(None)
def slot_batch(n):
    """n walked planes, every second one the transposed kind, cycling through KEPT_SIZES: 48 x 48, 64 x 64, 51 x 47, 52 x 48, 40 x 40, 32 x 32."""
    return [(tp.changed_plane if k % 2 else tp.kept_plane)(*tp.KEPT_SIZES[(k // 2 + 2 * (k % 2)) % len(tp.KEPT_SIZES)]) for k in range(n)]


SLOT_SIZES = (TIE_SLOTS - 1, TIE_SLOTS, TIE_SLOTS + 1, 40)
GRID = dict(g=24, cell=30, per_row=16, pad=(1, 1))             # 481 columns: odd, like the pixel count of every grid plane
WATCH_CASES = {254: (127, 0), 255: (127, 1), 256: (128, 0), 257: (128, 1), 258: (129, 0)}     # census -> (glyphs, of them with a third stroke)


@functools.lru_cache(None)
def watch_plane(census):
    n, triples = WATCH_CASES[census]
    return tp.grid_plane(n, triples=triples, **GRID)


@functools.lru_cache(None)
def dense_batch():
    """20 dense planes (census 257, 258 and 262; w * h odd) in turn with 20 sparse walked ones."""
    dense = [watch_plane(257), watch_plane(258), tp.grid_plane(131, **dict(GRID, pad=(3, 5)))]
    out = []
    for k in range(20):
        out += [dense[k % 3], slot_batch(40)[k]]
    return out


RELEVANCE = {      # name -> (plane, planes walked).  50 rows x 70 columns, coef 0.7: 0.64 x 3500 = 2240 = 0.7 x 3200 = 0.7 x (64 x 50)
    "differs": (lambda: tp.relevance_plane(50, 70, 60, 46, 55, 39, third=False), 1),
    "just below": (lambda: tp.relevance_plane(50, 70, 63, 50, 59, 46), 1),
    "at": (lambda: tp.relevance_plane(50, 70, 64, 50, 60, 46), 1),
    "above": (lambda: tp.relevance_plane(50, 70, 65, 50, 61, 46), 0),
}
REL_P = {"differs": 60 * 46, "just below": 63 * 50, "at": 64 * 50, "above": 65 * 50}


@functools.lru_cache(None)
def resize_batch():
    """(planes, kinds) of 64 x 48: between planes whose pools stay, two whose pools change size in the walk and one whose pool changes a node."""
    kinds = ("free", "kept", "noise 0", "rect", "changed", "noise 2", "settled", "free")
    make = {"free": lambda: tp.free_plane(48, 64), "kept": lambda: tp.kept_plane(64, 48), "noise 0": lambda: tp.noise_plane(0), "rect": lambda: tp.rect_plane(48, 64, 9, 7, 20, 16),
            "changed": lambda: tp.changed_plane(64, 48), "noise 2": lambda: tp.noise_plane(2), "settled": lambda: tp.settled_plane(48, 64)}
    return [make[k]() for k in kinds], kinds


@functools.lru_cache(None)
def many_batch():
    """CHUNK + 1 planes of 32 x 32: changed at 0, CHUNK - 1 and CHUNK, settled at CHUNK / 2, else tie-free ones, every fifth with a rectangle."""
    planes, kinds = [], []
    for k in range(CHUNK + 1):
        if k in (0, CHUNK - 1, CHUNK):
            planes.append(tp.changed_plane(32, 32, 20, 20)); kinds.append("changed")
        elif k == CHUNK // 2:
            planes.append(tp.settled_plane(32, 32, 20, 6, 6)); kinds.append("settled")
        elif k % 5 == 1:
            planes.append(tp.rect_plane(32, 32, 2 + k % 11, 3 + k % 7, 12 + k % 3, 14)); kinds.append("rect")
        else:
            planes.append(tp.free_plane(32, 32)); kinds.append("free")
    return planes, kinds


# =================================================================================================================================
# CPU: every plane has the property it was made for -- on the oracle and the census alone
# =================================================================================================================================
_FACTS = {}


def facts(oracle, plane, prm=None):
    """(ambiguous, nodes, census, parents of the census, pool keys under sibling modes 0, 1, 2), once per plane."""
    prm = prm or tp.PRM
    k = (plane.shape, plane.tobytes(), prm["overlap_coef"])
    if k not in _FACTS:
        r = [oracle.detect_plane(plane, sibling_mode=m, **prm) for m in (0, 1, 2)]
        tr = r[0]["tree"]
        pools = tuple(tuple(sorted(int(x["tree"].nodes[i]["key"]) for i in x["pool"])) for x in r)
        cen, parents = tp.watch_census(tr.nodes, tr.root, plane.shape[0], plane.shape[1], prm["overlap_coef"])
        _FACTS[k] = (r[0]["ambiguous"], len(tr.nodes), cen, len(parents), pools)
    return _FACTS[k]


def kind_of(oracle, plane, prm=None):
    """'free' (no tie), 'settled' (one two-way tie, one pool), 'kept' / 'changed' (the reference's pool is the largest-key pool -- the first pass's -- / is
    not), with ' x n' for n ties."""
    amb, _, cen, parents, (p0, p1, p2) = facts(oracle, plane, prm)
    if amb == 0:
        return "free"
    if p0 == p1 == p2:
        return "settled" if (amb, cen) == (1, 2) else "equal x %d" % amb
    return ("kept" if p0 == p2 else "changed") + ("" if amb == 1 else " x %d" % amb)


def test_the_constants_the_planes_were_made_for():
    assert (ALT_CAP, WATCH_CAP, TIE_SLOTS) == (64, 256, 16)
    with open(os.path.join(CSRC, "er_nms.inl")) as fh:
        src = fh.read()
    for kernel in ("k_cand_prefix", "k_cand_reprefix", "k_alt_list", "k_tie_slots"):            # one workgroup of CHUNK lanes each
        assert re.search(r"__launch_bounds__\(%d\)\s+void\s+%s\(" % (CHUNK, kernel), src) and re.search(r"%s, dim3\(1\), dim3\(%d\)" % (kernel, CHUNK), src)
    assert "base += %d" % CHUNK in src


def test_census_on_a_table_counted_by_hand():
    """Root 200 x 200.  P (100 x 100) has children of 60 x 60, 55 x 60, 100 x 31 (> 0.3 of it: three watched) and 50 x 50, 30 x 100 (not).  Q (100 x 90) has
    one child above 0.3: none.  R (180 x 180) has two children above 0.3, but 0.3 x 32400 = 9720 < 0.64 x 40000 = 25600 holds only at coef 0.3 --
    at coef 0.8 (x 32400 = 25920) its ties are irrelevant, and 150 x 175 = 26250 > 0.8 x 32400 are its only children that large."""
    rows = [(200, 200, 0), (100, 100, 0), (60, 60, 1), (55, 60, 1), (100, 31, 1), (50, 50, 1), (30, 100, 1), (100, 90, 0), (60, 60, 7), (20, 20, 7),
            (180, 180, 0), (150, 175, 10), (175, 150, 10), (10, 10, 10)]
    t = np.zeros(len(rows), [("w", np.uint16), ("h", np.uint16), ("parent", np.int32)])
    for i, r in enumerate(rows):
        t[i] = r
    t["parent"][0] = -1
    assert tp.watch_census(t, 0, 200, 200, 0.3) == (5, [1, 10]) and tp.tie_parents(t, 0, 0.3) == {1: 3, 10: 2}
    assert tp.watch_census(t, 0, 200, 200, 0.8) == (0, []) and tp.tie_parents(t, 0, 0.8) == {10: 2}
    assert tp.watch_census(t, 0, 203, 200, 0.8) == (2, [10])            # 0.64 x 203 x 200 = 25984 > 25920


def test_glyph_planes_are_kept_changed_or_settled(oracle):
    for size in tp.KEPT_SIZES:
        k, c = tp.kept_plane(*size), tp.changed_plane(*size)
        assert k.shape == c.shape == (size[1], size[0])
        for plane, kind in ((k, "kept"), (c, "changed"), (tp.flipped(k, "lr"), "kept"), (tp.flipped(k, "ud"), "kept"), (tp.flipped(k, "r180"), "changed")):
            amb, nodes, cen, parents, pools = facts(oracle, plane)
            assert (amb, nodes, cen, parents) == (1, 7, 2, 1) and kind_of(oracle, plane) == kind
            assert len(pools[0]) == len(pools[1]) == len(pools[2]) == 1 and pools[1] != pools[2]        # same size, another node
    for plane in (tp.settled_plane(), tp.settled_plane(transposed=True), tp.settled_plane(32, 32, 20, 6, 6), tp.settled_plane(48, 64)):
        amb, nodes, cen, parents, pools = facts(oracle, plane)
        assert (amb, nodes, cen, parents) == (1, 10, 2, 1) and pools[0] == pools[1] == pools[2] and len(pools[0]) == 1
    assert kind_of(oracle, tp.kept_plane(64, 48)) == "kept" and kind_of(oracle, tp.changed_plane(64, 48)) == "changed"
    amb, _, cen, parents, _ = facts(oracle, two_glyph_plane())
    assert (amb, cen, parents) == (2, 4, 2) and kind_of(oracle, two_glyph_plane()) == "changed x 2"
    assert len(set(facts(oracle, two_glyph_plane())[4])) == 3
    assert two_glyph_plane().shape == (48, 48)
    # the tie-free planes: none or one candidate
    assert facts(oracle, tp.free_plane(48, 48)) == (0, 1, 0, 0, ((), (), ()))
    amb, nodes, cen, parents, pools = facts(oracle, tp.rect_plane(48, 48, 5, 7, 14, 12))
    assert (amb, cen) == (0, 0) and len(pools[0]) == 1


def test_alt_batches(oracle):
    for name, (n_settled, walked, n_walked) in ALT_CASES.items():
        planes, kinds = alt_batch(n_settled, walked)
        assert all(p.shape == (48, 48) for p in planes) and len(planes) == len(kinds) == n_settled + n_settled // 3 + (3 if walked else 0)
        got = [kind_of(oracle, p) for p in planes]
        assert [g for g, k in zip(got, kinds) if k == "settled"] == ["settled"] * n_settled
        assert all(g == "free" for g, k in zip(got, kinds) if k == "free") and kinds.count("free") == n_settled // 3
        wk = [g for g, k in zip(got, kinds) if k == "walked"]
        assert wk == {"": [], "two": ["changed x 2"] * 3, "one": ["kept", "changed", "changed"]}[walked]
        # planes for the list: one relevant two-way tie.  Those beyond NMS_ALT_CAP keep their tie; so do the walked ones, listed or not
        listable = n_settled + (3 if walked == "one" else 0)
        assert n_walked == max(0, listable - ALT_CAP) + (3 if walked else 0)
        assert kinds[0] == ("walked" if walked else "settled") and kinds[-1] == ("walked" if walked else kinds[-1])
    assert ALT_CASES["81"][2] == TIE_SLOTS + 1 and ALT_CASES["61 + 3 of one tie"][0] + 3 == ALT_CAP


def test_slot_batches(oracle):
    for n in SLOT_SIZES:
        b = slot_batch(n)
        kinds = [kind_of(oracle, p) for p in b]
        assert len(b) == n and kinds == ["kept", "changed"] * (n // 2) + ["kept"] * (n % 2)
        widths = {p.shape[1] for p in b}
        assert {48, 52, 51} <= widths and any(w % 16 == 0 for w in widths) and any(w % 16 and w % 4 == 0 for w in widths) and any(w % 4 for w in widths)
        assert len({p.shape for p in b}) >= 6
        # 51 x 47 and 47 x 51 (2397 pixels: not a multiple of 256) in front of other planes
        at = [i for i, p in enumerate(b) if p.shape[0] * p.shape[1] == 51 * 47]
        assert at and at[0] < n - 1 and (51 * 47) % 256 != 0
    assert SLOT_SIZES == (15, 16, 17, 40)


def test_watch_planes_by_the_census(oracle):
    for census, (n, triples) in WATCH_CASES.items():
        p = watch_plane(census)
        amb, nodes, cen, parents, pools = facts(oracle, p)
        assert cen == census == 2 * n + triples and parents == n and amb >= n
        assert pools[0] != pools[1] and pools[0] != pools[2]               # neither key rule gives the reference's pool
        assert (p.shape[0] * p.shape[1]) % 64 != 0
    assert sorted(WATCH_CASES) == [WATCH_CAP - 2, WATCH_CAP - 1, WATCH_CAP, WATCH_CAP + 1, WATCH_CAP + 2]
    b = dense_batch()
    assert len(b) == 40
    for k, p in enumerate(b):
        cen = facts(oracle, p)[2]
        assert (cen > WATCH_CAP and (p.shape[0] * p.shape[1]) % 64 != 0) if k % 2 == 0 else cen == 2
        assert kind_of(oracle, p) not in ("free", "settled")
    assert 20 - TIE_SLOTS >= 4                                              # dense planes without a slot, whichever planes get the slots
    assert len({p.shape for p in b[0::2]}) == 3


def test_relevance_planes(oracle):
    rows, cols, coef = 50, 70, 0.7
    assert 64 * 50 * 7 == 64 * rows * cols // 10 and (64 * rows * cols) % 10 == 0                 # equality, in integers: 0.7 x 3200 = 0.64 x 3500
    for name, (make, walked) in RELEVANCE.items():
        p = make()
        assert p.shape == (rows, cols)
        r = oracle.detect_plane(p, **tp.REL_PRM)
        tr = r["tree"]
        ties = tp.tie_parents(tr.nodes, tr.root, coef)
        assert len(ties) == 1
        P = tr.nodes[next(iter(ties))]
        assert int(P["w"]) * int(P["h"]) == REL_P[name] and list(ties.values()) == [2 if name == "differs" else 3]
        side = REL_P[name] * 70 - 64 * rows * cols
        assert (side < 0, side == 0, side > 0) == {"differs": (1, 0, 0), "just below": (1, 0, 0), "at": (0, 1, 0), "above": (0, 0, 1)}[name]
        amb, _, cen, parents, pools = facts(oracle, p, tp.REL_PRM)
        assert amb >= 1 and cen == (0 if name == "above" else list(ties.values())[0])
        assert walked == (0 if name == "above" else 1)
        if name == "differs":
            assert pools[1] != pools[2] and len(pools[0]) == 1
        else:
            assert pools[0] == pools[1] == pools[2]           # "above": the claim the rule rests on; below it by a column and at it the rule is on the safe side
    # the largest box the pool takes on this plane is smaller than what a chain start under the other three P's must exceed
    assert 56 * 39 * 10 < 7 * 63 * 50 and 56 * 10 == 8 * cols and 39 * 10 < 8 * rows == 40 * 10


def test_resize_batch(oracle):
    planes, kinds = resize_batch()
    assert all(p.shape == (48, 64) for p in planes)
    got = [kind_of(oracle, p) for p in planes]
    assert [g.split(" x ")[0] for g in got] == ["free", "kept", "changed", "free", "changed", "changed", "settled", "free"]
    first = [len(facts(oracle, p)[4][2]) for p in planes]                  # the first pass: largest key
    ref = [len(facts(oracle, p)[4][0]) for p in planes]
    assert first == [0, 1, 70, 1, 1, 77, 1, 0] and ref == [0, 1, 72, 1, 1, 76, 1, 0]        # grows by two, shrinks by one; the records behind them move
    for seed, a, b in ((0, 70, 72), (1, 69, 70), (2, 77, 76), (3, 73, 72), (5, 81, 80)):
        amb, _, cen, _, pools = facts(oracle, tp.noise_plane(seed))
        assert (len(pools[2]), len(pools[0])) == (a, b) and amb > 1 and 16 <= cen <= 26 < WATCH_CAP


def test_many_batch(oracle):
    planes, kinds = many_batch()
    assert len(planes) == CHUNK + 1 and all(p.shape == (32, 32) for p in planes)
    assert [i for i, k in enumerate(kinds) if k == "changed"] == [0, CHUNK - 1, CHUNK] and kinds.index("settled") == CHUNK // 2
    for want, name in (("changed", "changed"), ("settled", "settled"), ("free", "free"), ("free", "rect")):
        assert {kind_of(oracle, p) for p, k in zip(planes, kinds) if k == name} == {want}
    pool = [len(facts(oracle, p)[4][0]) for p in planes]
    assert set(pool) == {0, 1} and 0 in pool[:CHUNK] and 1 in pool[:CHUNK] and kinds.count("rect") > 100       # cand_base is not constant


# =================================================================================================================================
# GPU
# =================================================================================================================================
STAGES_NMS = 1 | 2                           # STAGE_EXTRACT | STAGE_NMS


def _ctx(S, monkeypatch, replay, planes, prm=None, cascade_paths=None):
    """A context for the largest plane of `planes` and as many planes a call, made under STR_ER_REPLAY = replay."""
    prm = prm or tp.PRM
    monkeypatch.setenv("STR_ER_REPLAY", replay)
    f = S.ERFilter(prm["step"], prm["min_area"], prm["max_area"], prm["stability_t"], prm["overlap_coef"], max_width=max(p.shape[1] for p in planes),
                   max_height=max(p.shape[0] for p in planes), max_frames=(len(planes) + 5) // 6)
    if cascade_paths:
        f.load_cascade(0, cascade_paths[0])
        f.load_cascade(1, cascade_paths[1])
    return f


def _run(f, planes, stages=STAGES_NMS, as_list=True):
    """(result, growth of planes_walked)."""
    before = f.tie_stats()["planes_walked"]
    res = f.detect_planes_list(planes, stages, want_nodes=True) if as_list else f.detect_planes(np.stack(planes), stages, want_nodes=True)
    return res, f.tie_stats()["planes_walked"] - before


def _check(oracle, res, planes, prm=None, cascades=None):
    assert len(res.planes) == len(planes)
    for p, img in zip(res.planes, planes):
        assert (p.width, p.height) == (img.shape[1], img.shape[0])
        check_plane_against_oracle(oracle, p, img, cascades, **(prm or tp.PRM))


def _bytes(res):
    return res.info.tobytes(), res.cands.tobytes(), tuple(p.nodes.tobytes() for p in res.planes)


REPLAYS = ("host", "gpu")


@pytest.mark.gpu
@pytest.mark.parametrize("replay", REPLAYS)
@pytest.mark.parametrize("name", list(ALT_CASES))
def test_gpu_alt_list(S, oracle, monkeypatch, replay, name):
    """Case 1.  The list is filled through an atomic counter: which planes get it differs from run to run, the pools and the count do not."""
    n_settled, walked, n_walked = ALT_CASES[name]
    planes, kinds = alt_batch(n_settled, walked)
    f = _ctx(S, monkeypatch, replay, planes)
    res, delta = _run(f, planes, as_list=False)
    _check(oracle, res, planes)
    assert delta == n_walked
    assert all(p.ambiguous >= 1 for p, k in zip(res.planes, kinds) if k != "free")
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SLOT_SIZES)
def test_gpu_slots_and_exports(S, oracle, monkeypatch, n):
    """Case 2: host mode (slots, both export kernels, the arena) against the oracle, and gpu mode (nothing exported) equal to it byte for byte."""
    planes = slot_batch(n)
    got = {}
    for replay in REPLAYS:
        f = _ctx(S, monkeypatch, replay, planes)
        res, delta = _run(f, planes)
        assert delta == n
        _check(oracle, res, planes)
        got[replay] = _bytes(res)
        f.close()
    assert got["host"] == got["gpu"]


@pytest.mark.gpu
def test_gpu_exports_from_device_planes_at_an_odd_pitch(S, oracle, monkeypatch):
    """Case 2, device planes used where they lie: plane k starts 1 + k bytes into its rows of pitch w + 7 + 2 k, so the copy width of export_plane follows
    pointer and pitch -- the byte copy for widths 48 and 64 too."""
    planes = slot_batch(TIE_SLOTS + 1)
    f = _ctx(S, monkeypatch, "host", planes)
    hip_malloc, hip_memcpy, hip_free = f.L.hipMalloc, f.L.hipMemcpy, f.L.hipFree
    hip_malloc.argtypes, hip_memcpy.argtypes, hip_free.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    refs, parts, at = [], [], 0
    for k, p in enumerate(planes):
        h, w = p.shape
        pitch = w + 7 + 2 * k if k % 3 else w + 16 - w % 16          # (every third one at a pitch of 16 n: 4-byte or 16-byte moves where the width allows)
        buf = np.full(pitch * h + 64, 0xA5, np.uint8)
        off = 1 + k if k % 3 else 0
        for y in range(h):
            buf[off + y * pitch:off + y * pitch + w] = p[y]
        refs.append((at + off, w, h, pitch))
        parts.append(buf)
        at += (len(buf) + 255) // 256 * 256
    d = C.c_void_p()
    assert hip_malloc(C.byref(d), at) == 0
    try:
        pos = 0
        for buf in parts:
            assert hip_memcpy(d.value + pos, buf.ctypes.data, len(buf), 1) == 0           # (hipMemcpyHostToDevice)
            pos += (len(buf) + 255) // 256 * 256
        before = f.tie_stats()["planes_walked"]
        res = f.detect_planes_list_device([(d.value + o, w, h, pitch) for o, w, h, pitch in refs], STAGES_NMS, want_nodes=True)
        assert f.tie_stats()["planes_walked"] - before == len(planes)
        _check(oracle, res, planes)
        assert _bytes(res) == _bytes(f.detect_planes_list(planes, STAGES_NMS, want_nodes=True))
    finally:
        hip_free(d)
        f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("replay", REPLAYS)
@pytest.mark.parametrize("census", list(WATCH_CASES))
def test_gpu_watch_list(S, oracle, monkeypatch, replay, census):
    """Case 3: a plane on either side of the watch list, alone and between sparse tie planes."""
    p = watch_plane(census)
    batch = [tp.kept_plane(51, 47, 30, 26), tp.changed_plane(), p, tp.changed_plane(51, 47, 30, 26), tp.kept_plane(32, 32, 20, 20)]
    f = _ctx(S, monkeypatch, replay, batch)
    res, delta = _run(f, [p])
    _check(oracle, res, [p])
    assert delta == 1 and res.planes[0].ambiguous >= WATCH_CASES[census][0]
    res, delta = _run(f, batch)
    _check(oracle, res, batch)
    assert delta == 5
    f.close()


@pytest.mark.gpu
def test_gpu_dense_planes_between_sparse_ones(S, oracle, monkeypatch):
    """Case 3, host mode: 40 tie planes on 16 slots -- at least four of the 20 dense ones lie in the arena, each stamp area of 4 w h bytes with w h odd, with
    sparse planes behind them."""
    planes = dense_batch()
    f = _ctx(S, monkeypatch, "host", planes)
    res, delta = _run(f, planes)
    _check(oracle, res, planes)
    assert delta == 40
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("replay", REPLAYS)
def test_gpu_relevance_rule(S, oracle, monkeypatch, replay):
    """Case 4: a three-way tie (two-way in "differs", whose pools differ) is nothing for the opposite-rule pass, so the plane is walked iff k_nms counts
    the tie as relevant."""
    planes = {name: make() for name, (make, _) in RELEVANCE.items()}
    f = _ctx(S, monkeypatch, replay, list(planes.values()), tp.REL_PRM)
    for name, p in planes.items():
        res, delta = _run(f, [p])
        _check(oracle, res, [p], tp.REL_PRM)
        assert delta == RELEVANCE[name][1], name
        assert res.planes[0].ambiguous >= 1
    res, delta = _run(f, list(planes.values()), as_list=False)
    _check(oracle, res, list(planes.values()), tp.REL_PRM)
    assert delta == 3
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("replay", REPLAYS)
def test_gpu_pools_that_change_size(S, oracle, oracle_cascades, cascade_paths, monkeypatch, replay):
    """Case 5: every stage, the shipped cascades.  The pools of planes 2 and 5 grow by two and shrink by one in the walk, plane 4's changes a node: new bases
    and the redo list of k_cand_reprefix, the records of the planes between and behind them shifted by k_cand_move."""
    planes, kinds = resize_batch()
    f = _ctx(S, monkeypatch, replay, planes, cascade_paths=cascade_paths)
    res, delta = _run(f, planes, S.STAGE_ALL, as_list=False)
    _check(oracle, res, planes, cascades=oracle_cascades)
    assert delta == 4
    assert [len(p.cands) for p in res.planes] == [0, 1, 72, 1, 1, 76, 1, 0]
    again, delta = _run(f, planes, S.STAGE_ALL, as_list=False)
    assert delta == 4 and _bytes(again) == _bytes(res)
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("replay", REPLAYS)
def test_gpu_more_planes_than_a_scan_turn(S, oracle, oracle_cascades, cascade_paths, monkeypatch, replay):
    """Case 6: 1025 planes in one call; the pools of planes 0, 1023 and 1024 change in the walk."""
    planes, kinds = many_batch()
    f = _ctx(S, monkeypatch, replay, planes, cascade_paths=cascade_paths)
    res, delta = _run(f, planes, S.STAGE_ALL, as_list=False)
    assert delta == 3
    _check(oracle, res, planes, cascades=oracle_cascades)
    assert int(res.cands["plane"][-1]) == CHUNK and len(res.cands) == sum(len(p.cands) for p in res.planes) > 100
    f.close()


@pytest.mark.gpu
def test_gpu_small_large_small_on_one_context(S, oracle, monkeypatch):
    """Case 7, host mode: the arena and the scratch grow with the 40 planes and with the dense plane and are reused by the small batch."""
    small, large, dense = slot_batch(TIE_SLOTS - 1), slot_batch(40), [watch_plane(WATCH_CAP + 2)]
    f = _ctx(S, monkeypatch, "host", large + dense)
    first = {}
    for name, planes in (("small", small), ("large", large), ("dense", dense), ("small", small), ("large", large), ("dense", dense), ("small", small)):
        res, delta = _run(f, planes)
        assert delta == len(planes)
        if name not in first:
            _check(oracle, res, planes)
            first[name] = _bytes(res)
        assert _bytes(res) == first[name], name
    f.close()
