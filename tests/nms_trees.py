"""Hand-made component trees for test_nms_edges.py: one description, two forms (the binding's node table, the oracle's Tree).

A tree is an (n, 7) integer array of (level, area, x, y, w, h, parent) rows and a key per row.  NmsTree checks that it is a tree
str_er_nms_tree accepts and that an extraction could have produced: one root, levels strictly rising towards it, every box nested in
its parent's, unique keys, boxes of at most 4096 x 4096.  The oracle's child lists hold the children of a parent in ascending table
index: the contract of str_er_nms_tree at sibling_order = 0 (include/str_er.h)."""
import numpy as np

from oracle.oracle import NODE_DTYPE as ORACLE_NODE, Tree

LEVEL, AREA, X, Y, W, H, PARENT = range(7)
FILL_BOXES = ((11, 12), (12, 13), (13, 14))           # a chain of three: 132 / 156 / 182 pixels, 132 / 182 > 0.7


class NmsTree:
    def __init__(self, rows, keys=None, seed=0, root_as_self=False):
        r = np.array(rows, np.int64).reshape(-1, 7)
        n = len(r)
        idx = np.arange(n)
        is_root = (r[:, PARENT] < 0) | (r[:, PARENT] == idx)
        assert is_root.sum() == 1, "one root"
        self.root = int(np.nonzero(is_root)[0][0])
        r[self.root, PARENT] = -1
        self.rows = r
        self.keys = np.random.default_rng(seed).permutation(n) if keys is None else np.array(keys, np.int64)
        self.root_as_self = root_as_self
        self._validate()

    def __len__(self):
        return len(self.rows)

    def _validate(self):
        r, n = self.rows, len(self.rows)
        assert len(self.keys) == n and len(np.unique(self.keys)) == n and self.keys.min() >= 0 and self.keys.max() < 2 ** 31
        assert (r[:, LEVEL] >= 0).all() and (r[:, LEVEL] <= 255).all()
        assert (r[:, W] >= 1).all() and (r[:, H] >= 1).all() and (r[:, W] <= 4096).all() and (r[:, H] <= 4096).all()
        assert (r[:, X] >= 0).all() and (r[:, Y] >= 0).all() and (r[:, X] + r[:, W] <= 65535).all() and (r[:, Y] + r[:, H] <= 65535).all()
        assert (r[:, AREA] >= 1).all() and (r[:, AREA] <= r[:, W] * r[:, H]).all()          # a region has no more pixels than its box
        c = np.arange(n) != self.root
        p = r[c, PARENT]
        assert (p >= 0).all() and (p < n).all()
        assert (r[p, LEVEL] > r[c, LEVEL]).all(), "a parent's level is above its child's"    # (hence no cycles)
        assert ((r[c, X] >= r[p, X]) & (r[c, Y] >= r[p, Y]) & (r[c, X] + r[c, W] <= r[p, X] + r[p, W]) &
                (r[c, Y] + r[c, H] <= r[p, Y] + r[p, H])).all(), "a child's box is nested in its parent's"

    # ---- the two forms ----------------------------------------------------------------------------------------------------------
    def table(self, dtype):
        """The binding's NODE_DTYPE table; the root's parent is -1 or, with root_as_self, its own index."""
        r = self.rows
        t = np.zeros(len(r), dtype)
        t["key"], t["area"], t["level"] = self.keys, r[:, AREA], r[:, LEVEL]
        t["x"], t["y"], t["w"], t["h"], t["parent"] = r[:, X], r[:, Y], r[:, W], r[:, H], r[:, PARENT]
        if self.root_as_self:
            t["parent"][self.root] = self.root
        return t

    def oracle_tree(self):
        r, n = self.rows, len(self.rows)
        nd = np.zeros(n, ORACLE_NODE)
        for f, col in (("level", LEVEL), ("area", AREA), ("x", X), ("y", Y), ("w", W), ("h", H), ("parent", PARENT)):
            nd[f] = r[:, col]
        nd["key"] = self.keys
        child, nxt = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
        par = r[:, PARENT]
        for i in range(n - 1, -1, -1):                     # prepended in descending order: ascending lists
            if par[i] >= 0:
                nxt[i] = child[par[i]]
                child[par[i]] = i
        nd["child"], nd["next"] = child, nxt
        return Tree(nd, self.root, n, 0)

    # ---- variants ---------------------------------------------------------------------------------------------------------------
    def _reordered(self, order):
        """New row j is old row order[j]: parents renumbered, every node keeps its key."""
        n = len(self.rows)
        new_of_old = np.empty(n, np.int64)
        new_of_old[order] = np.arange(n)
        r = self.rows[order].copy()
        has = r[:, PARENT] >= 0
        r[has, PARENT] = new_of_old[r[has, PARENT]]
        return NmsTree(r, self.keys[order], root_as_self=self.root_as_self)

    def permuted(self, seed):
        """The same tree with its rows in a random order: children come before and after their parents."""
        return self._reordered(np.random.default_rng(seed).permutation(len(self.rows)))

    def with_root_at(self, where):
        """The same tree with the root's row moved to table index `where` (the other rows keep their order)."""
        rest = [i for i in range(len(self.rows)) if i != self.root]
        return self._reordered(np.array(rest[:where] + [self.root] + rest[where:], np.int64))

    def respelled(self, root_as_self):
        return NmsTree(self.rows, self.keys, root_as_self=root_as_self)

    def padded(self, n_fill=4200, seed=77):
        """At least n_fill more nodes under the root, so that the table has more than 4096 rows.  Chains of three where the levels
        below the root leave room for them (the tree's own levels are used: no new level appears), single nodes otherwise.  The
        filler is not inert -- its chains are pooled, it may compete for a small root -- the oracle runs on the padded tree too."""
        r = self.rows
        root = r[self.root]
        assert root[W] >= 14 and root[H] >= 14 and root[LEVEL] >= 1, "the root has room for the filler"
        below = sorted(set(r[r[:, LEVEL] < root[LEVEL], LEVEL].tolist()))
        rng = np.random.default_rng(seed)
        n0, out = len(r), []
        if len(below) >= 3:
            for k in range((n_fill + 2) // 3):
                lv = sorted(rng.choice(below, 3, replace=False).tolist())
                x, y = root[X] + int(rng.integers(0, root[W] - 13)), root[Y] + int(rng.integers(0, root[H] - 13))
                base = n0 + 3 * k
                for j, (w, h) in enumerate(FILL_BOXES):
                    out.append((lv[j], w * h, x, y, w, h, base + j + 1 if j < 2 else self.root))
        else:
            lv = below[0] if below else 0
            for k in range(n_fill):
                w, h = FILL_BOXES[k % 3]
                out.append((lv, w * h, root[X] + int(rng.integers(0, root[W] - 13)), root[Y] + int(rng.integers(0, root[H] - 13)), w, h, self.root))
        keys = np.concatenate([self.keys, self.keys.max() + 1 + rng.permutation(len(out))])
        t = NmsTree(np.concatenate([r, np.array(out, np.int64)]), keys, root_as_self=self.root_as_self)
        assert len(t) > 4096 + 3
        return t


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def ref_pool(oracle, t, rows, cols, min_area=120, max_area=900000, stability_t=2, overlap_coef=0.7, mode=0):
    """oracle.nms on the tree: (pool as table indices in ascending key order, the oracle's tie count)."""
    pool, amb = oracle.nms(t.oracle_tree(), rows, cols, 8, min_area, max_area, stability_t, overlap_coef, mode)
    assert len(set(pool.tolist())) == len(pool)
    return sorted(pool.tolist(), key=lambda i: int(t.keys[i])), amb


def pool_keys(t, pool):
    return sorted(int(t.keys[i]) for i in pool)


# ---- builders shared by the families -----------------------------------------------------------------------------------------------
def chain_rows(boxes, parent, first_index, x=0, y=0, level0=0, level_step=1, areas=None):
    """A chain, leaf first: boxes[k] = (w, h) at (x, y); member k has index first_index + k and level level0 + k * level_step; the
    last member hangs on `parent`.  area = w * h unless given."""
    out = []
    for k, (w, h) in enumerate(boxes):
        out.append((level0 + k * level_step, w * h if areas is None else areas[k], x, y, w, h, first_index + k + 1 if k + 1 < len(boxes) else parent))
    return out


def random_tree(n, seed, coef_num=7, coef_den=10, levels=None, root_box=4000, root_level=None):
    """n nodes, every one hung on a random earlier node of the table that has a level to spare.  The child's box is one of four
    kinds: its area just above coef x the parent's, exactly at it (where the parent's width allows, else just below), the
    parent's own box, or an eighth of each side.  levels: the levels that may be used (default: all 256)."""
    rng = np.random.default_rng(seed)
    levels = list(range(256)) if levels is None else sorted(levels)
    top = len(levels) - 1 if root_level is None else levels.index(root_level)
    rows = [(levels[top], max(1, root_box * root_box // 2), 0, 0, root_box, root_box, -1)]
    rank = [top]                                    # index of a node's level in `levels`
    open_ = [0] if top > 0 else []                  # nodes that can still take a child
    while len(rows) < n:
        assert open_, "levels exhausted"
        p = open_[int(rng.integers(0, len(open_)))] if rng.random() < 0.7 else open_[-1 - int(rng.integers(0, min(8, len(open_))))]
        _, _, px, py, pw, ph, _ = rows[p]
        kind = int(rng.integers(0, 4))
        if kind == 0:
            w, h = min(pw, pw * coef_num // coef_den + 1), ph
        elif kind == 1:
            w, h = max(1, pw * coef_num // coef_den), ph
        elif kind == 2:
            w, h = pw, ph
        else:
            w, h = max(1, pw // 8), max(1, ph // 8)
        if rng.random() < 0.5:
            w, h = min(w, pw), min(ph, h)
            if kind < 2 and rng.random() < 0.5:           # trim the height instead of the width
                w, h = pw, (min(ph, ph * coef_num // coef_den + 1) if kind == 0 else max(1, ph * coef_num // coef_den))
        x, y = px + int(rng.integers(0, pw - w + 1)), py + int(rng.integers(0, ph - h + 1))
        lr = max(0, rank[p] - 1 - int(rng.integers(0, 3)) * int(rng.random() < 0.3))
        area = max(1, int(w * h * rng.uniform(0.3, 1.0)))
        rows.append((levels[lr], area, x, y, w, h, p))
        rank.append(lr)
        if lr > 0:
            open_.append(len(rows) - 1)
    return NmsTree(rows, seed=seed)
