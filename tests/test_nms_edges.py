"""non_maximum_supression on hand-made trees at k_nms's own edges (csrc/er_nms.inl).

Every tree below is made up for one part of the kernel: the overlap test exactly at the coefficient, sibling ties under the three tie
rules, the counting sort over 256 levels, the stability walk next to the root, the acceptance filter at each bound, a pool on
either side of NMS_SORT_CAP.  Each runs as it is (at most NMS_LDS_CAP = 4096 nodes: node facts in registers and LDS) and again
with more than 4096 nodes hung under the root (the tables in memory).  The CPU section proves on the oracle alone that each tree
reaches the edge it was made for; the GPU section compares str_er_nms_tree with oracle.nms on the same tree, `==`."""
import ctypes as C
import functools
from typing import NamedTuple

import numpy as np
import pytest

from nms_trees import FILL_BOXES, H, LEVEL, NmsTree, W, chain_rows, pool_keys, random_tree, ref_pool

EINVAL, ECAPACITY = -1, -7                 # STR_ER_EINVAL, STR_ER_ECAPACITY (include/str_er.h)
NMS_CAP = 4096                             # NMS_LDS_CAP and NMS_SORT_CAP (csrc/er_nms.inl)
CTX_CAPS = {}                              # extra Params of every context made here (none: the tables grow on demand)


class P(NamedTuple):
    """The parameters of a context that the NMS reads."""
    min_area: int = 120
    max_area: int = 900000
    T: int = 2
    coef: float = 0.7


_padded = functools.lru_cache(None)(lambda t: t.padded())
_permuted = functools.lru_cache(None)(lambda t, seed: t.permuted(seed))
_REF = {}


def _ref(oracle, t, rows, cols, prm=P(), mode=0):
    """oracle.nms, once per (tree, plane size, parameters, sibling mode)."""
    k = (id(t), rows, cols, prm, mode)
    if k not in _REF:
        _REF[k] = (t,) + ref_pool(oracle, t, rows, cols, prm.min_area, prm.max_area, prm.T, prm.coef, mode)
    return _REF[k][1], _REF[k][2]


def _both(t):
    """The tree as it is (LDS path) and padded past 4096 nodes (memory path)."""
    assert len(t) <= NMS_CAP
    return (t, _padded(t))


# =================================================================================================================================
# 1. the overlap test at exact quotients
# =================================================================================================================================
COEFS = {"0.7": (7, 10, 0.7), "0.5": (1, 2, 0.5), "0.25": (1, 4, 0.25), "0.9": (9, 10, 0.9), "1/3": (1, 3, 1.0 / 3.0)}
SIDES = (-1, 0, 1)


def _between(w, h, pw, ph):
    """A box strictly between (w, h) and (pw, ph), nested in both ways, whose stability beats the start's in the chain (w, h), (w, h), B, P, P -- or None."""
    if w < pw and h < ph and w * ph != h * pw:
        return (pw, h) if h * pw > w * ph else (w, ph)
    if w == pw and h < ph - 1:
        return (pw, ph - 1)
    if h == ph and w < pw - 1:
        return (pw - 1, ph)
    return None


@functools.lru_cache(None)
def boundary_boxes(num, den, lo, hi, side):
    """A parent box (pw, ph), lo <= pw, ph <= hi, and a box (w, h) nested in it of target + side pixels, where target * den == pw * ph * num exactly."""
    for pw in range(lo, hi + 1):
        for ph in range(lo, hi + 1):
            if (pw * ph * num) % den:
                continue
            a = pw * ph * num // den + side
            for w in range(pw, 0, -1):
                h = a // w
                if a % w == 0 and h <= ph and 0.5 < w / h < 1.9 and _between(w, h, pw, ph):
                    return (pw, ph), (w, h)
    raise AssertionError("no boundary boxes")


@functools.lru_cache(None)
def overlap_tree(name, side):
    """The boundary at three places, the start's box one pixel below (side -1), exactly at (0) and one pixel above (+1) coef x the box
    it is tested against.  Returns (tree, {place: its node indices}).
      'start': X -> P -> Q (= P's box): above, X's chain is X, P, Q and X is pooled; else X and P, Q stay short of T + 1 members.
      'two up': X -> A (= X's box) -> B -> P -> Q: the test that decides is the one of the chain X, A, B against P; above, B or A wins the
                longer chain (B's stability is the largest by construction), else X, the only member of X, A, B with two members above it.
      'root':  X -> A (= X's box) -> the root: above, the chain takes the root and X is pooled."""
    num, den, _ = COEFS[name]
    (rw, rh), (w, h) = boundary_boxes(num, den, 400, 460, side)
    rows = [(20, rw * rh, 0, 0, rw, rh, -1)]
    place = {"root": [1, 2], "start": [3, 4, 5], "two up": [6, 7, 8, 9, 10]}
    rows += chain_rows([(w, h), (w, h)], 0, 1, x=0, y=0)
    (pw, ph), (w, h) = boundary_boxes(num, den, 100, 140, side)
    rows += chain_rows([(w, h), (pw, ph), (pw, ph)], 0, 3, x=150, y=0)
    rows += chain_rows([(w, h), (w, h), _between(w, h, pw, ph), (pw, ph), (pw, ph)], 0, 6, x=150, y=150)
    t = NmsTree(rows, seed=11)
    r = t.rows
    a_start, a_par = int(r[3, W] * r[3, H]), int(r[4, W] * r[4, H])
    assert a_start * den == a_par * num + side * den and int(r[1, W] * r[1, H]) * den == rw * rh * num + side * den
    return t, place


# =================================================================================================================================
# 2. ties
# =================================================================================================================================
def _tie_parent(rows, k, x0, y0, root=0):
    """P (100 x 100) under the root, Q (= P's box) above it, and k two-node chains x_j -> c_j (one box, > 0.7 of P's) under P: every one of
    them passes on P, the winner's chain is x, c, P, Q and its x is pooled."""
    p = len(rows)
    rows.append((5, 9000, x0, y0, 100, 100, p + 1))
    rows.append((6, 9500, x0, y0, 100, 100, root))
    for j in range(k):
        w, h = 97 - j % 8, 97 - (j // 8) % 8
        x, y = x0 + (3 * j) % (100 - w + 1), y0 + (5 * j) % (100 - h + 1)
        i = len(rows)
        rows.append((0, w * h - 50, x, y, w, h, i + 1))
        rows.append((1 + j % 3, w * h - 20, x, y, w, h, p))
    return p


def _stacked(rows, x0, y0, n_mid=3, root=0):
    """Ties on ties: P (100 x 100) <- c_i (95 x 95) <- d_i1 (90 x 90, passes on c_i AND on P) and d_i2 (80 x 82, passes on c_i only), each d
    above an x of its own box.  Where d_i2 wins the tie at c_i, c_i's chain does not compete for P."""
    p = len(rows)
    rows.append((8, 9000, x0, y0, 100, 100, p + 1))
    rows.append((9, 9500, x0, y0, 100, 100, root))
    for i in range(n_mid):
        c = len(rows)
        rows.append((5 + i % 2, 8000, x0 + i, y0 + i, 95, 95, p))
        for (w, h) in ((90, 90), (80, 82)):
            j = len(rows)
            rows.append((0, w * h - 30, x0 + i + 1, y0 + i + 2, w, h, j + 1))
            rows.append((1 + i % 3, w * h - 10, x0 + i + 1, y0 + i + 2, w, h, c))


@functools.lru_cache(None)
def ties_tree():
    """Parents with 2, 3 and 64 passing child chains and three stacked ties."""
    rows = [(50, 1000000, 0, 0, 4000, 4000, -1)]
    for n, k in enumerate((2, 3, 64, 2, 3)):
        _tie_parent(rows, k, 200 * n, 0)
    for n in range(3):
        _stacked(rows, 200 * n, 300, n_mid=2 + n)
    return NmsTree(rows, seed=21)


@functools.lru_cache(None)
def two_way_tree():
    """50 parents with two passing child chains each, and nothing else that ties."""
    rows = [(50, 1000000, 0, 0, 4000, 4000, -1)]
    for n in range(50):
        _tie_parent(rows, 2, 150 * (n % 10), 150 * (n // 10))
    return NmsTree(rows, seed=22)


@functools.lru_cache(None)
def wide_root_tree():
    """A 1000 x 1000 root with 2000 children: 300 two-node chains that pass on it (one slot of the proposal table takes them all), 200
    chains of three and 1500 single nodes that do not."""
    rng = np.random.default_rng(23)
    rows = [(10, 400000, 0, 0, 1000, 1000, -1)]
    kinds = rng.permutation(np.repeat([0, 1, 2], [300, 200, 1500]))
    for kind in kinds:
        i = len(rows)
        if kind == 0:
            w, h = int(rng.integers(850, 1001)), int(rng.integers(850, 1001))
            x, y = int(rng.integers(0, 1000 - w + 1)), int(rng.integers(0, 1000 - h + 1))
            rows += [(int(rng.integers(0, 4)), w * h // 2, x, y, w, h, i + 1), (int(rng.integers(4, 9)), w * h // 2 + 9, x, y, w, h, 0)]
        elif kind == 1:
            rows += chain_rows(FILL_BOXES, 0, i, x=int(rng.integers(0, 900)), y=int(rng.integers(0, 900)), level0=int(rng.integers(0, 5)))
        else:
            rows.append((int(rng.integers(0, 10)), 200, int(rng.integers(0, 900)), int(rng.integers(0, 900)), 20, 30, 0))
    return NmsTree(rows, seed=23)


TIE_TREES = {"ties": ties_tree, "two-way": two_way_tree, "wide root": wide_root_tree}
TIE_PLANE = 4000                 # rows = cols of the ties' calls: every box below the roots passes the size filter


# =================================================================================================================================
# 3. random nested trees
# =================================================================================================================================
RANDOM_SIZES = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 20000)
RANDOM_SEEDS = (0, 1, 2)


@functools.lru_cache(None)
def random_case(n, seed):
    return random_tree(n, 1000 * seed + n)


# =================================================================================================================================
# 4. levels
# =================================================================================================================================
GAP_LEVELS = (0, 3, 4, 127, 128, 252, 255)


@functools.lru_cache(None)
def level_trees():
    out = {}
    # one chain over all 256 levels: 20 x 30 at the leaf, a pixel more each way per level, in a shuffled table
    out["256 levels"] = NmsTree(chain_rows([(20 + k, 30 + k) for k in range(256)], -1, 0), seed=41).permuted(41)
    out["gaps"] = random_tree(600, 42, levels=GAP_LEVELS, root_box=600)
    for name, lv in (("all at 0", 0), ("all at 254", 254)):
        rng = np.random.default_rng(43 + lv)
        rows = [(255, 2000, 0, 0, 50, 50, -1)]
        for _ in range(1000):                              # 30 .. 50 pixels a side: some pass on the root (0.7 x 2500 = 1750), most do not
            w, h = int(rng.integers(30, 51)), int(rng.integers(30, 51))
            rows.append((lv, int(w * h * rng.uniform(0.2, 1.0)), int(rng.integers(0, 50 - w + 1)), int(rng.integers(0, 50 - h + 1)), w, h, 0))
        out[name] = NmsTree(rows, seed=44 + lv).permuted(45 + lv)
    # levels 2 and 3 share a group of four in the scan: 500 nodes at each (the hole a wrong start leaves is 500 slots wide)
    rng = np.random.default_rng(46)
    rows = [(255, 2000, 0, 0, 50, 50, -1)]
    for k in range(1000):
        w, h = int(rng.integers(30, 51)), int(rng.integers(30, 51))
        rows.append((2 + k % 2, int(w * h * rng.uniform(0.2, 1.0)), int(rng.integers(0, 50 - w + 1)), int(rng.integers(0, 50 - h + 1)), w, h, 0))
    out["500 at 2, 500 at 3"] = NmsTree(rows, seed=47).permuted(48)
    return out


LEVEL_PRMS = (P(), P(T=0), P(T=1))
LEVEL_PLANE = 400                   # rows = cols of the level trees' calls


# =================================================================================================================================
# 5. stability
# =================================================================================================================================
STAB_T = (0, 1, 2, 3, 5)


def _equal_stability_heights(T):
    """Heights (the width is 30 throughout) of a chain of T + 2 members whose two stabilities are equal and finite: a_0 / (a_T - a_0) ==
    a_1 / (a_T+1 - a_1) exactly (8 and 8 at T = 1, 4 and 4 above), the areas differ, and a_0 / a_T+1 > 0.7."""
    if T == 1:
        return [64, 72, 81]
    return [40, 44] + [45, 46, 48][:T - 2] + [50, 55]


@functools.lru_cache(None)
def stability_forest(T):
    """Chains under a root too large to be taken.  Returns (tree, {name: indices of the chain, leaf first})."""
    rng = np.random.default_rng(50 + T)
    rows = [(200, 1000000, 0, 0, 4000, 4000, -1)]
    note = {}

    def add(name, heights):
        i = len(rows)
        note[name] = list(range(i, i + len(heights)))
        rows.extend(chain_rows([(30, h) for h in heights], 0, i, x=40 * (len(note) % 90), y=100 * (len(note) // 90), level_step=1 + len(note) % 3))

    for L in (T, T + 1, T + 2):
        if L >= 1:
            add("length %d" % L, [40 + k for k in range(L)])
    add("one box", [40] * (T + 3))                                      # every stability is +inf
    add("+inf above a finite one", [40, 41] + [42] * (T + 2))              # the lowest member's is finite, +inf from the third on
    add("+inf twice", [40, 40, 41, 41, 42, 42][:T + 2] + [42] * 3)
    if T >= 1:
        add("equal", _equal_stability_heights(T))
        add("largest in the middle", [40, 48, 49, 55] if T == 1 else [40, 44] + [45, 46, 47][:T - 2] + [48, 49, 55])        # 5, 8.8 (48 at T = 1), less
    for k in range(40):
        add("random %d" % k, (40 + np.cumsum(rng.integers(0, 3, int(rng.integers(max(T, 1), T + 8))))).tolist())
    return NmsTree(rows, seed=50 + T), note


@functools.lru_cache(None)
def root_chain(L, root_level=9):
    """A tree that is one chain of L members, the last of them the root: 30 x 40 at the leaf, a pixel higher per member.  With rows =
    cols = 100 every member passes the filter; the members within T of the root have no stability."""
    rows = chain_rows([(30, 40 + k) for k in range(L)], -1, 0, level0=root_level - (L - 1))
    return NmsTree(rows, seed=60 + L).permuted(60 + L)


def root_chain_lengths(T):
    return sorted({1, 2} | {L for L in (T, T + 1, T + 2, T + 3) if L >= 1})


# =================================================================================================================================
# 6. the acceptance filter
# =================================================================================================================================
FILTER_PRM = P()
SMALL_PRM = P(min_area=4)
# (w, h, area, pooled): w / h against 2.0 and 0.10, area against min_area = 120 and max_area = 900000; rows = cols = 2000
FILTER_CASES = ((40, 20, 700, False), (39, 20, 700, True), (10, 100, 900, False), (11, 100, 900, True), (30, 40, 120, False), (30, 40, 121, True),
                (1000, 1000, 899999, True), (1000, 1000, 900000, False), (1000, 1000, 900001, False), (1599, 1000, 5000, True), (1000, 1599, 5000, True),
                (1600, 1000, 5000, False), (1000, 1600, 5000, False))
# min_area = 4: the 1 x 10 box of the issue, and areas 4 and 5
SMALL_CASES = ((1, 10, 10, False), (1, 9, 9, True), (4, 2, 8, False), (3, 2, 6, True), (2, 2, 4, False), (2, 3, 5, True))
SIDE_PLANES = (5, 10, 7, 1080)              # 0.8 x n: 4.0 and 8.0 (integers), 5.6 and 864.0000000000001 in exact arithmetic -- 864.0 as a double
SIDE_SIZES = (2, 3, 4, 5, 6, 7, 8, 9, 862, 863, 864, 865)


def _case_tree(cases):
    """A chain of three members of one box (+inf: the lowest is the chain's winner) per case, under a 4096 x 4096 root."""
    rows = [(200, 1000000, 0, 0, 4096, 4096, -1)]
    first = []
    for k, (w, h, area) in enumerate(cases):
        first.append(len(rows))
        rows.extend(chain_rows([(w, h)] * 3, 0, len(rows), x=1650 * (k % 2), y=0, level0=k % 5, areas=[area, area, area]))
    return NmsTree(rows, seed=61), first


@functools.lru_cache(None)
def filter_tree():
    return _case_tree([c[:3] for c in FILTER_CASES])


@functools.lru_cache(None)
def small_tree():
    return _case_tree([c[:3] for c in SMALL_CASES])


@functools.lru_cache(None)
def side_tree():
    """Square boxes of SIDE_SIZES pixels a side, area = w * h (above min_area = 4 from 3 x 3 on)."""
    return _case_tree([(s, s, s * s) for s in SIDE_SIZES])


def side_expected(n):
    """Sides below 0.8 n, by hand for the planes of the issue."""
    return {5: (3,), 10: (3, 4, 5, 6, 7), 7: (3, 4, 5), 1080: (3, 4, 5, 6, 7, 8, 9, 862, 863)}[n]


# =================================================================================================================================
# 7. pool size
# =================================================================================================================================
COMB_SIZES = (4095, 4096, 4097, 6000)


@functools.lru_cache(None)
def comb(n):
    """n chains of three under a 4000 x 4000 root: one pooled node per chain.  The three members of a chain are n rows apart."""
    rows = [(10, 1000000, 0, 0, 4000, 4000, -1)]
    for j, (w, h) in enumerate(FILL_BOXES):
        for k in range(n):
            rows.append((j + k % 3, w * h, 14 * (k % 280), 16 * (k // 280), w, h, 1 + (j + 1) * n + k if j < 2 else 0))
    return NmsTree(rows, seed=70)


# =================================================================================================================================
# CPU: the trees reach their edges
# =================================================================================================================================
def test_helper_refuses_what_no_extraction_gives():
    good = [(5, 100, 0, 0, 20, 20, -1), (3, 50, 2, 2, 10, 10, 0), (1, 20, 3, 3, 5, 5, 1)]
    NmsTree(good)
    for bad in ([(5, 100, 0, 0, 20, 20, -1), (3, 50, 2, 2, 10, 10, -1)],                              # two roots
                [(5, 100, 0, 0, 20, 20, 1), (3, 50, 2, 2, 10, 10, 0)],                                # none
                [(5, 100, 0, 0, 20, 20, -1), (5, 50, 2, 2, 10, 10, 0)],                               # equal levels
                [(5, 100, 0, 0, 20, 20, -1), (3, 50, 12, 2, 10, 10, 0)],                              # the box leaves its parent's
                [(5, 100, 0, 0, 20, 20, -1), (3, 50, 2, 2, 0, 10, 0)],                                # an empty box
                [(5, 100, 0, 0, 20, 20, -1), (3, 101, 2, 2, 10, 10, 0)],                              # more pixels than the box has
                [(5, 100, 0, 0, 4097, 20, -1)], [(256, 100, 0, 0, 20, 20, -1)]):
        with pytest.raises(AssertionError):
            NmsTree(bad)
    with pytest.raises(AssertionError):
        NmsTree(good, keys=[1, 1, 2])
    t = NmsTree(good, keys=[7, 3, 5])
    o = t.permuted(3).oracle_tree()
    assert sorted(o.nodes["key"].tolist()) == [3, 5, 7]
    for tree in (ties_tree(), _padded(ties_tree()), _permuted(ties_tree(), 5)):                     # child lists: ascending table index
        nd = tree.oracle_tree().nodes
        for p in range(len(nd)):
            kids, c = [], int(nd[p]["child"])
            while c >= 0:
                kids.append(c)
                c = int(nd[c]["next"])
            assert kids == sorted(kids) and all(int(nd[k]["parent"]) == p for k in kids)
        assert sum(int(x["parent"]) >= 0 for x in nd) == len(nd) - 1
    assert not (np.diff(ties_tree().keys) > 0).all() and len(_padded(ties_tree())) > NMS_CAP         # the keys are not in table order


def test_overlap_trees_sit_on_the_coefficient(oracle):
    for name, (num, den, coef) in COEFS.items():
        assert coef == num / den
        pools = {}
        for side in SIDES:
            t, place = overlap_tree(name, side)
            r = t.rows
            a_s, a_p = int(r[3, W] * r[3, H]), int(r[4, W] * r[4, H])
            assert (a_s / a_p > coef) == (side > 0) and (a_s * den > a_p * num) == (side > 0)       # the double quotient says what the integers say
            assert (a_s / a_p == coef) == (side == 0)
            for tree in _both(t):
                pool, amb = _ref(oracle, tree, 2000, 2000, P(coef=coef))
                pools[side, tree is t] = {p: sorted(set(pool) & set(idx)) for p, idx in place.items()}
        for plain in (True, False):
            for p in ("start", "two up", "root"):
                # exactly at the coefficient is "not above": the pools of -1 and 0 agree, +1 gives another one
                assert pools[-1, plain][p] == pools[0, plain][p] != pools[1, plain][p], (name, p)
            assert pools[1, plain]["start"] == [3] and pools[0, plain]["start"] == []
            assert pools[1, plain]["root"] == [1] and pools[0, plain]["root"] == []
            assert pools[0, plain]["two up"] == [6] and 6 not in pools[1, plain]["two up"]


def test_tie_trees_depend_on_the_rule_and_on_the_table_order(oracle):
    three_ways = moved = 0
    for name, make in TIE_TREES.items():
        t = make()
        for tree in _both(t) + (_permuted(t, 7), _padded(_permuted(t, 7))):
            by_mode = [pool_keys(tree, _ref(oracle, tree, TIE_PLANE, TIE_PLANE, mode=m)[0]) for m in (0, 1, 2)]
            assert all(_ref(oracle, tree, TIE_PLANE, TIE_PLANE, mode=m)[1] > 0 for m in (0, 1, 2)) and all(len(p) > 0 for p in by_mode)
            three_ways += by_mode[0] != by_mode[1] != by_mode[2] != by_mode[0]
        a, b = _ref(oracle, t, TIE_PLANE, TIE_PLANE)[0], _ref(oracle, _permuted(t, 7), TIE_PLANE, TIE_PLANE)[0]
        moved += pool_keys(t, a) != pool_keys(_permuted(t, 7), b)
        for m in (1, 2):                                  # the key rules do not read the table order
            assert pool_keys(t, _ref(oracle, t, TIE_PLANE, TIE_PLANE, mode=m)[0]) == pool_keys(_permuted(t, 7), _ref(oracle, _permuted(t, 7), TIE_PLANE, TIE_PLANE, mode=m)[0])
    assert three_ways >= 6 and moved == len(TIE_TREES)
    # the two-way family: one losing chain per tied parent, with the filler too
    for tree in _both(two_way_tree()):
        assert all(_ref(oracle, tree, TIE_PLANE, TIE_PLANE, mode=m)[1] == 50 for m in (0, 1, 2))
    # 2, 3 and 64 passing chains: the oracle counts the losers
    assert _ref(oracle, ties_tree(), TIE_PLANE, TIE_PLANE)[1] >= 1 + 2 + 63 + 1 + 2
    # the wide root: hundreds of chains pass on one node
    t = wide_root_tree()
    r = t.rows
    kids = np.nonzero(r[:, 6] == t.root)[0]
    assert len(kids) == 2000 and _ref(oracle, t, TIE_PLANE, TIE_PLANE)[1] == (r[kids, W] * r[kids, H] > 700000).sum() - 1 >= 250
    # stacked: who wins below changes who competes above -- the x under a d_i2 is pooled where d_i2 won its tie (its chain then stops below P):
    # under the smallest-key rule where its key is the smaller one, under the largest-key rule in all the other places
    s = ties_tree()
    lows = [i for i in range(len(s)) if (s.rows[i, W], s.rows[i, H]) == (80, 82) and s.rows[i, LEVEL] == 0]
    got = {m: set(_ref(oracle, s, TIE_PLANE, TIE_PLANE, mode=m)[0]) & set(lows) for m in (0, 1, 2)}
    assert len(lows) == 9 and got[1] | got[2] == set(lows) and not got[1] & got[2] and got[1] and got[2]


def test_random_trees_have_ties_and_pools(oracle):
    for n in RANDOM_SIZES:
        good = 0
        for seed in RANDOM_SEEDS:
            t = random_case(n, seed)
            assert len(t) == n
            pool, amb = _ref(oracle, t, 4000, 4000)
            good += amb > 0 and len(pool) > 0
        # (a tie takes a parent and two children, a pooled node at T = 2 a chain of three: no tree of 1, 2 or 3 nodes has both)
        assert good >= 1 or n <= 3, n
    t = random_case(20000, 0)
    pools = [pool_keys(t, _ref(oracle, t, 4000, 4000, mode=m)[0]) for m in (0, 1, 2)]
    assert _ref(oracle, t, 4000, 4000)[1] > 1000 and pools[0] != pools[1] != pools[2] != pools[0] and len(pools[0]) > 100
    r = t.rows
    c = np.arange(len(r)) != t.root
    pa, ca = (r[r[c, 6], W] * r[r[c, 6], H]), r[c, W] * r[c, H]
    assert (ca * 10 == pa * 7).sum() > 100 and (ca == pa).sum() > 1000 and ((ca * 10 > pa * 7) & (ca < pa)).sum() > 1000 and (ca * 10 < pa * 7).sum() > 1000


def test_level_trees_use_the_levels_they_claim(oracle):
    lt = level_trees()
    assert sorted(lt["256 levels"].rows[:, LEVEL].tolist()) == list(range(256)) and len(lt["256 levels"]) == 256
    assert set(lt["gaps"].rows[:, LEVEL].tolist()) == set(GAP_LEVELS)
    assert set(_padded(lt["gaps"]).rows[:, LEVEL].tolist()) == set(GAP_LEVELS)                       # the filler adds no level
    for name, lv in (("all at 0", 0), ("all at 254", 254)):
        for tree in _both(lt[name]):
            assert sorted(set(tree.rows[:, LEVEL].tolist())) == [lv, 255] and (tree.rows[:, LEVEL] == 255).sum() == 1
    r = lt["500 at 2, 500 at 3"].rows
    assert (r[:, LEVEL] == 2).sum() == 500 == (r[:, LEVEL] == 3).sum() and len(r) == 1001
    for name, t in lt.items():
        sizes = [len(_ref(oracle, t, LEVEL_PLANE, LEVEL_PLANE, prm)[0]) for prm in LEVEL_PRMS]
        assert sizes[1] > 0 and sizes[2] > 0, (name, sizes)                                          # (T = 2 pools nothing where no chain has three members)
    assert len(_ref(oracle, lt["256 levels"], LEVEL_PLANE, LEVEL_PLANE)[0]) > 5                     # the long chain breaks into many
    assert _ref(oracle, lt["all at 0"], LEVEL_PLANE, LEVEL_PLANE, P(T=1))[1] > 50                    # and the flat ones tie at the root


def test_stability_trees_decide_by_equal_and_infinite_stabilities(oracle):
    for T in STAB_T:
        t, note = stability_forest(T)
        for tree in _both(t):
            pool = set(_ref(oracle, tree, TIE_PLANE, TIE_PLANE, P(T=T))[0])
            for L in (T, T + 1, T + 2):
                if L >= 1:
                    assert bool(pool & set(note["length %d" % L])) == (L >= T + 1)
            assert pool & set(note["one box"]) == {note["one box"][0]}
            inf = note["+inf above a finite one"]
            assert pool & set(inf) == {inf[0] if T == 0 else inf[2]}                              # the first member whose T-th ancestor repeats its box
            assert len(pool & set(note["+inf twice"])) == 1
            if T >= 1:
                eq = note["equal"]
                a = [int(tree.rows[i, W] * tree.rows[i, H]) for i in eq]
                assert len(eq) == T + 2 and a[0] / (a[T] - a[0]) == a[1] / (a[T + 1] - a[1]) and a[0] < a[1] and a[0] / a[-1] > 0.7
                assert pool & set(eq) == {eq[0]}                                                    # equal stabilities: the lowest
                mid = note["largest in the middle"]
                assert pool & set(mid) == {mid[1]}
        for L in root_chain_lengths(T):
            c = root_chain(L)
            for tree in _both(c):
                pool = set(_ref(oracle, tree, 100, 100, P(T=T))[0])
                own = pool & set(range(L))
                assert len(own) == (1 if L >= T + 1 else 0), (T, L)
                if own and T > 0:                                 # the winner has T members above it: it is not within T of the root
                    win = own.pop()
                    assert tree.rows[win, LEVEL] <= 9 - T
    assert set(_ref(oracle, root_chain(1), 100, 100, P(T=0))[0]) == {0} and _ref(oracle, root_chain(1), 100, 100, P(T=2))[0] == []
    assert _ref(oracle, root_chain(1), 40, 100, P(T=0))[0] == []                                    # 40 rows: the root is too high to be accepted


def test_filter_trees_sit_on_every_bound(oracle):
    for make, cases, prm in ((filter_tree, FILTER_CASES, FILTER_PRM), (small_tree, SMALL_CASES, SMALL_PRM)):
        t, first = make()
        for tree in _both(t):
            pool = set(_ref(oracle, tree, 2000, 2000, prm)[0])
            assert pool & set(range(len(t))) == {first[k] for k, c in enumerate(cases) if c[3]}
    assert 40 / 20 == 2.0 and 1 / 10 == 0.10 and 10 / 100 == 0.10 and 1599 < 0.8 * 2000 == 1600
    assert 0.8 * 5 == 4.0 and 0.8 * 10 == 8.0 and 5 < 0.8 * 7 < 6 and 0.8 * 1080 == 864.0
    t, first = side_tree()
    for n in SIDE_PLANES:
        for rows, cols in ((n, 2000), (2000, n)):
            for tree in _both(t):
                pool = set(_ref(oracle, tree, rows, cols, SMALL_PRM)[0]) & set(range(len(t)))
                assert pool == {first[SIDE_SIZES.index(s)] for s in side_expected(n)}, (rows, cols)


def test_combs_cross_the_sort_capacity(oracle):
    for n in COMB_SIZES:
        for t in (comb(n), _permuted(comb(n), n)):
            pool, amb = _ref(oracle, t, TIE_PLANE, TIE_PLANE)
            assert len(pool) == n and amb == 0 and len(t) == 3 * n + 1 > NMS_CAP
            assert set(t.rows[pool, W] * t.rows[pool, H]) == {FILL_BOXES[0][0] * FILL_BOXES[0][1]}      # one per chain: its lowest member
            assert (np.diff(pool) < 0).sum() > n // 3                                                 # ranked order is not table order
    assert COMB_SIZES[0] < NMS_CAP + 1 and COMB_SIZES[1] == NMS_CAP and COMB_SIZES[2] == NMS_CAP + 1


def test_root_place_and_spelling_do_not_matter(oracle):
    t = ties_tree()
    base = pool_keys(t, _ref(oracle, t, TIE_PLANE, TIE_PLANE)[0])
    for where in (0, len(t) // 2, len(t) - 1):
        m = t.with_root_at(where)
        assert m.root == where
        for spell in (False, True):
            s = m.respelled(spell)
            assert s.table(np.dtype([(f, "<i8") for f in ("key", "area", "level", "x", "y", "w", "h", "parent")]))["parent"][where] == (where if spell else -1)
            assert pool_keys(s, _ref(oracle, s, TIE_PLANE, TIE_PLANE)[0]) == base                    # (siblings keep their table order)


# =================================================================================================================================
# GPU
# =================================================================================================================================
@pytest.fixture(scope="module")
def ctx(S):
    """Contexts by (parameters, sibling_order), made on first use; 64 x 64 x 1 frame: their tables start small and grow with the trees."""
    made = {}

    def get(prm=P(), order=0):
        if (prm, order) not in made:
            made[prm, order] = S.ERFilter(params=S.Params(thresh_step=8, min_area=prm.min_area, max_area=prm.max_area, stability_t=prm.T, overlap_coef=prm.coef,
                                                          max_width=64, max_height=64, max_frames=1, sibling_order=order, **CTX_CAPS))
        return made[prm, order]

    yield get
    for f in made.values():
        f.close()


def _check(ctx, S, oracle, t, rows, cols, prm=P(), order=0, exact_amb=False):
    """str_er_nms_tree == oracle.nms: the pool in ascending key order, the tie count zero or not (or as a number)."""
    want, ramb = _ref(oracle, t, rows, cols, prm, order)
    pool, amb = ctx(prm, order).non_maximum_supression(t.table(S.NODE_DTYPE), rows, cols)
    assert pool.tolist() == want, (len(pool), len(want), sorted(set(pool.tolist()) ^ set(want))[:8])
    assert (np.diff(t.keys[pool]) > 0).all()
    assert (amb == 0) == (ramb == 0), (amb, ramb)
    if exact_amb:
        assert amb == ramb
    return pool, amb


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(COEFS))
def test_gpu_overlap_at_exact_quotients(ctx, S, oracle, name):
    """as * den == ap * num, a pixel less and a pixel more: at a chain's start, two members up, and where the chain would take the root."""
    prm = P(coef=COEFS[name][2])
    for side in SIDES:
        t, place = overlap_tree(name, side)
        for tree in _both(t):
            pool, _ = _check(ctx, S, oracle, tree, 2000, 2000, prm)
            assert (3 in pool) == (1 in pool) == (6 not in pool) == (side > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("order", (0, 1, 2))
@pytest.mark.parametrize("name", list(TIE_TREES))
def test_gpu_ties_under_the_three_rules(ctx, S, oracle, name, order):
    """2, 3, 64 and hundreds of passing child chains, ties on ties; table index, smallest key, largest key; the table as built and shuffled."""
    t = TIE_TREES[name]()
    for tree in _both(t) + (_permuted(t, 7), _padded(_permuted(t, 7))):
        _, amb = _check(ctx, S, oracle, tree, TIE_PLANE, TIE_PLANE, order=order, exact_amb=name == "two-way")
        assert amb > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", RANDOM_SIZES)
def test_gpu_random_nested_trees(ctx, S, oracle, n):
    """Children just above the coefficient, exactly at it, of the parent's own box and small; node counts around the wave, the workgroup and NMS_LDS_CAP."""
    for seed in RANDOM_SEEDS:
        for order in (0, 1, 2):
            _check(ctx, S, oracle, random_case(n, seed), 4000, 4000, order=order)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("256 levels", "gaps", "all at 0", "all at 254", "500 at 2, 500 at 3"))
def test_gpu_levels(ctx, S, oracle, name):
    """The counting sort over the levels: all 256 in one chain, gaps around the scan's groups of four, everything at one level."""
    t = level_trees()[name]
    for tree in _both(t):
        for prm in LEVEL_PRMS:
            _check(ctx, S, oracle, tree, LEVEL_PLANE, LEVEL_PLANE, prm)


@pytest.mark.gpu
@pytest.mark.parametrize("T", STAB_T)
def test_gpu_stability(ctx, S, oracle, T):
    """Chains of T, T + 1 and T + 2 members, chains that end in the root, +inf and equal finite stabilities; stability_t 0, 1, 2, 3, 5."""
    prm = P(T=T)
    t, note = stability_forest(T)
    for tree in _both(t) + (_permuted(t, T),):
        pool, _ = _check(ctx, S, oracle, tree, TIE_PLANE, TIE_PLANE, prm)
    for L in root_chain_lengths(T):
        for tree in _both(root_chain(L)):
            _check(ctx, S, oracle, tree, 100, 100, prm)
    _check(ctx, S, oracle, root_chain(1), 40, 100, prm)                     # a root-only tree whose root is too high to be accepted


@pytest.mark.gpu
def test_gpu_acceptance_filter(ctx, S, oracle):
    """w / h at 2.0 and 0.10, area at min_area and max_area, h and w at 0.8 x rows and 0.8 x cols: each bound from both sides."""
    for make, cases, prm in ((filter_tree, FILTER_CASES, FILTER_PRM), (small_tree, SMALL_CASES, SMALL_PRM)):
        t, first = make()
        for tree in _both(t):
            pool, _ = _check(ctx, S, oracle, tree, 2000, 2000, prm)
            assert set(pool.tolist()) & set(range(len(t))) == {first[k] for k, c in enumerate(cases) if c[3]}
    t, _ = side_tree()
    for n in SIDE_PLANES:
        for rows, cols in ((n, 2000), (2000, n)):
            for tree in _both(t):
                _check(ctx, S, oracle, tree, rows, cols, SMALL_PRM)


@pytest.mark.gpu
@pytest.mark.parametrize("n", COMB_SIZES)
def test_gpu_pool_sizes_around_the_sort_capacity(ctx, S, oracle, n):
    """4095, 4096, 4097 and 6000 pooled nodes: ranked out of LDS up to NMS_SORT_CAP, from memory above."""
    for t in (comb(n), _permuted(comb(n), n)):
        pool, amb = _check(ctx, S, oracle, t, TIE_PLANE, TIE_PLANE, exact_amb=True)
        assert len(pool) == n and amb == 0


@pytest.mark.gpu
def test_gpu_root_place_and_spelling(ctx, S, oracle):
    """The root first, in the middle and last in the table, its parent written as -1 and as its own index."""
    t = ties_tree()
    base = None
    for tree in _both(t):
        for where in (0, len(tree) // 2, len(tree) - 1):
            for spell in (False, True):
                s = tree.with_root_at(where).respelled(spell)
                assert s.table(S.NODE_DTYPE)["parent"][where] == (where if spell else -1)
                pool, _ = _check(ctx, S, oracle, s, TIE_PLANE, TIE_PLANE)
                keys = s.keys[pool].tolist()
                if where == 0 and not spell:
                    base = keys
                assert keys == base


@pytest.mark.gpu
def test_gpu_small_large_small_on_one_context(S, oracle):
    """A small tree, a large one and the small one again on a fresh context: the tables grow in between, the scratch of the large
    tree stays behind, and the answers are the same bytes."""
    cases = ((ties_tree(), random_case(20000, 1), TIE_PLANE), (wide_root_tree(), comb(6000), TIE_PLANE), (level_trees()["all at 254"], _padded(level_trees()["256 levels"]), LEVEL_PLANE),
             (stability_forest(2)[0], _padded(two_way_tree()), TIE_PLANE))
    for small, large, plane in cases:
        f = S.ERFilter(params=S.Params(thresh_step=8, min_area=120, max_area=900000, stability_t=2, overlap_coef=0.7, max_width=64, max_height=64, max_frames=1, **CTX_CAPS))
        got = []
        for t in (small, large, small, large):
            pool, amb = f.non_maximum_supression(t.table(S.NODE_DTYPE), plane, plane)
            assert pool.tolist() == _ref(oracle, t, plane, plane)[0]
            got.append((pool.tobytes(), amb))
        assert got[0] == got[2] and got[1] == got[3]
        f.close()


# ---- errors and sizing: str_er_nms_tree itself ---------------------------------------------------------------------------------------
def _raw(f, table, rows, cols, cap, with_pool=True):
    """str_er_nms_tree through the library handle: (return code, n_pool, pool buffer of max(cap, 1) entries set to -9 before the call)."""
    pool = np.full(max(cap, 1), -9, np.int32)
    n, amb = C.c_int32(-5), C.c_int32(-5)
    rc = f.L.str_er_nms_tree(f.h, table.ctypes.data, len(table), rows, cols, pool.ctypes.data if with_pool else None, cap, C.byref(n), C.byref(amb))
    return rc, n.value, pool


@pytest.mark.gpu
def test_gpu_nms_tree_refusals_and_sizing(ctx, S, oracle):
    """Two roots, no root, a parent out of range, an empty box, equal levels: STR_ER_EINVAL, and the context answers as before; cap
    below the pool: the count and the head of the answer; cap = 0 with a null buffer: the count."""
    f = ctx()
    good = ties_tree()
    tab = good.table(S.NODE_DTYPE)
    want = _ref(oracle, good, TIE_PLANE, TIE_PLANE)[0]
    assert len(want) > 8
    rc, n, full = _raw(f, tab, TIE_PLANE, TIE_PLANE, len(tab))
    assert rc == 0 and n == len(want) and full[:n].tolist() == want and (full[n:] == -9).all()
    child = int(np.nonzero(tab["parent"] == good.root)[0][0])
    leaf = int(np.nonzero(tab["level"] == 0)[0][0])

    def broken(kind):
        b = tab.copy()
        if kind == "two roots":
            b["parent"][child] = -1
        elif kind == "two roots, one its own parent":
            b["parent"][child] = child
        elif kind == "no root":
            b["parent"][good.root] = child
        elif kind == "parent out of range":
            b["parent"][leaf] = len(b)
        elif kind == "empty box":
            b["w"][leaf] = 0
        elif kind == "empty box, h":
            b["h"][leaf] = 0
        elif kind == "equal levels":
            b["level"][leaf] = b["level"][b["parent"][leaf]]
        return b

    for kind in ("two roots", "two roots, one its own parent", "no root", "parent out of range", "empty box", "empty box, h", "equal levels"):
        rc, n, pool = _raw(f, broken(kind), TIE_PLANE, TIE_PLANE, len(tab))
        assert rc == EINVAL and (pool == -9).all(), kind
        rc, n, again = _raw(f, tab, TIE_PLANE, TIE_PLANE, len(tab))
        assert rc == 0 and n == len(want) and again.tobytes() == full.tobytes(), kind
    for cap in (1, 5, len(want) - 1):
        rc, n, pool = _raw(f, tab, TIE_PLANE, TIE_PLANE, cap)
        assert rc == 0 and n == len(want) and pool[:cap].tolist() == want[:cap]
    rc, n, _ = _raw(f, tab, TIE_PLANE, TIE_PLANE, 0, with_pool=False)
    assert rc == 0 and n == len(want)
    rc, n, _ = _raw(f, tab, TIE_PLANE, TIE_PLANE, 4, with_pool=False)              # a capacity without a buffer
    assert rc == EINVAL
    rc, n, again = _raw(f, tab, TIE_PLANE, TIE_PLANE, len(tab))
    assert rc == 0 and again.tobytes() == full.tobytes()


@pytest.mark.gpu
def test_gpu_nms_tree_above_kept_cap(S, oracle):
    """A context with explicit capacities does not grow its tables: a tree of kept_cap nodes passes, one node more is STR_ER_ECAPACITY."""
    f = S.ERFilter(params=S.Params(thresh_step=8, min_area=120, max_area=900000, stability_t=2, overlap_coef=0.7, max_width=64, max_height=64, max_frames=1,
                                   kept_cap=1024, pool_cap=1024))
    fits, over = random_case(1024, 0), random_case(1025, 0)
    for _ in range(2):
        pool, _ = f.non_maximum_supression(fits.table(S.NODE_DTYPE), 4000, 4000)
        assert pool.tolist() == _ref(oracle, fits, 4000, 4000)[0] and len(pool) > 0
        rc, n, buf = _raw(f, over.table(S.NODE_DTYPE), 4000, 4000, 1025)
        assert rc == ECAPACITY and (buf == -9).all()
    f.close()
