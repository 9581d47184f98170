"""Made-up cascades and planes for tests/test_classify_edges.py.

The product's cascade_io.classifier_text writes what the reference writes: REAL rows with whole-number thresholds.  The writer here produces
any text CascadeBoost::load_classifier accepts -- REAL (`weight dim thresh cp cn`) and DISCRETE (`weight dim dir thresh`) rows, weights with
repr() precision, threshold tokens as arbitrary strings ("2.5", "nan", "-inf", "-0.0") -- and a numpy model of CascadeBoost::predict that
also says at WHICH stage a candidate was rejected, which neither the oracle nor the library reports.  The model is only used to tune stage
thresholds and to prove (on the CPU, together with the oracle) that a made-up cascade reaches the edge it was made for; what the GPU tests
compare the kernels with is the oracle alone.

Nothing here imports the product package.
"""
from __future__ import annotations

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)

# the classifier's NMS parameters under which a dark rectangle on a 200 background is pooled with its exact box
RECT_PRM = dict(step=8, min_area=0, max_area=900000, stability_t=0, overlap_coef=0.7)
RECT_H, RECT_W = 260, 400
CONST_DIMS = (0, 256, 512, 768)            # code 0 of the four cells: a constant tile puts 144 into each


def _f(v) -> str:
    return repr(float(v))


def threshold_tokens():
    """The thresholds the integer table is tested at: k, k +- 0.5 and the doubles next to k for k at both ends of a bin's possible counts (0 .. 144), then values past
    the integer table's clamp, a negative one, the negative zero, the infinities and NaN."""
    out = []
    for k in (0, 1, 2, 143, 144, 145):
        out += [_f(k), _f(k - 0.5), _f(k + 0.5), _f(np.nextafter(float(k), -np.inf)), _f(np.nextafter(float(k), np.inf))]
    return out + ["255", "256", "299.5", "300", "301", "1e9", "-1.5", "-0.0", "inf", "-inf", "nan"]


class Cascade:
    """One cascade file.  rows: REAL (weight, dim, thr_token, cp, cn); DISCRETE (weight, dim, dir, thr_token).  The file may hold more
    rows than stage_n announces (they are ignored by predict, but counted by the loaders)."""

    def __init__(self, real, stage_n, stage_thr, rows):
        self.real, self.stage_n, self.rows = bool(real), [int(n) for n in stage_n], list(rows)
        self.stage_thr = [str(t) for t in stage_thr]
        assert len(self.stage_thr) == len(self.stage_n) and sum(self.stage_n) <= len(self.rows)

    @property
    def shape(self):
        return len(self.stage_n), len(self.rows)

    def text(self) -> str:
        lines = ["boost_type " + ("REAL" if self.real else "DISCRETE"), "base_type DECISION_STUMP",
                 "num_of_iter " + " ".join(str(n) for n in self.stage_n), "threshold " + " ".join(self.stage_thr)]
        if self.real:
            lines += [f"{_f(w)} {int(d)} {t} {_f(cp)} {_f(cn)} " for (w, d, t, cp, cn) in self.rows]
        else:
            lines += [f"{_f(w)} {int(d)} {int(dr)} {t} " for (w, d, dr, t) in self.rows]
        return "\n".join(lines) + "\n"

    def with_stages(self, stage_n, stage_thr=None):
        return Cascade(self.real, stage_n, stage_thr or ["0"] * len(stage_n), self.rows)

    # ---- numpy model of CascadeBoost::predict (src/adaboost.cpp:507-542) ---------------------------------------------------------
    def stump_outputs(self, H):
        """(n_candidates, n_rows) outputs, REAL: fv < thr ? cp : cn; DISCRETE: (fv * dir < thr * dir ? 1 : -1) * weight."""
        dim = np.array([r[1] for r in self.rows], np.int64)
        fv = H[:, dim]
        with np.errstate(invalid="ignore"):
            if self.real:
                thr = np.array([float(r[2]) for r in self.rows])
                return np.where(fv < thr, np.array([r[3] for r in self.rows]), np.array([r[4] for r in self.rows]))
            thr = np.array([float(r[3]) for r in self.rows])
            d = np.array([float(int(r[2])) for r in self.rows])
            w = np.array([float(r[0]) for r in self.rows])
            return np.where(fv * d < thr * d, w, -w)

    def stage_sums(self, H):
        """(n_candidates, n_stages): every stage's sum, added in file order like `score_stage +=` (np.cumsum is sequential)."""
        out = self.stump_outputs(H)
        sums = np.zeros((len(H), len(self.stage_n)))
        off = 0
        for s, n in enumerate(self.stage_n):
            if n > 0:
                sums[:, s] = np.cumsum(out[:, off:off + n], axis=1)[:, -1]
            off += n
        return sums

    def predict(self, H):
        """(score, stage): score is -DBL_MAX and stage the index of the rejecting stage, or the last stage's sum and -1."""
        sums = self.stage_sums(H)
        thr = np.array([int(float(t)) for t in self.stage_thr], np.float64)        # (int)stod(...), src/adaboost.cpp:919
        rej = sums < thr[None, :]
        stage = np.where(rej.any(axis=1), rej.argmax(axis=1), -1)
        score = np.where(stage >= 0, -DBL_MAX, sums[:, -1])
        return score, stage


def classify_model(H, strong: Cascade, weak: Cascade):
    """ERFilter::classify (src/ER.cpp:507-528) on histograms: (cls, score_strong, score_weak, strong stage, weak stage); the weak
    cascade only speaks for what the strong one rejected (its stage is -2 where it was not asked)."""
    ss, st_s = strong.predict(H)
    sw_all, st_w_all = weak.predict(H)
    asked = st_s >= 0
    sw = np.where(asked, sw_all, 0.0)
    st_w = np.where(asked, st_w_all, -2)
    cls = np.where(~asked, 1, np.where(st_w == -1, 2, 0))
    return cls.astype(np.uint8), ss, sw, st_s, st_w


# ---- stump rows -------------------------------------------------------------------------------------------------------------------------
def useful_dims(H, min_distinct=4):
    """Histogram bins that take at least min_distinct different counts over the candidates: a stump elsewhere decides nothing."""
    return np.array([d for d in range(1024) if len(np.unique(H[:, d])) >= min_distinct], np.int64)


def _pair(rng):
    """(cp, cn) of opposite signs, like a trained stump's two outputs: a stage of one stump can then split its candidates at threshold 0."""
    a, b = float(rng.uniform(0.3, 3.0)), -float(rng.uniform(0.3, 3.0))
    return (a, b) if rng.random() < 0.5 else (b, a)


def random_rows(rng, H, n, real, dirs=(1, -1), thr_tokens=None):
    """n rows on useful dims; a threshold is one of the dim's own counts, or lies half or a quarter next to it, so that both sides occur.
    thr_tokens: tokens mixed in at every fourth row (NaN, infinities ...)."""
    dims = useful_dims(H)
    rows = []
    for i in range(n):
        d = int(dims[rng.integers(len(dims))])
        v = float(H[rng.integers(len(H)), d]) + float(rng.choice([0.0, 0.0, 0.5, -0.5, 0.25, 1.0]))
        t = _f(v)
        if thr_tokens and i % 4 == 3:
            t = str(thr_tokens[rng.integers(len(thr_tokens))])
        if real:
            cp, cn = _pair(rng)
            rows.append((float(rng.normal()), d, t, cp, cn))
        else:
            w = float(rng.uniform(0.3, 3.0)) * (1 if rng.random() < 0.8 else -1)
            rows.append((w, d, int(dirs[rng.integers(len(dirs))]), t))
    return rows


# ---- tuning the stage thresholds ---------------------------------------------------------------------------------------------------------
def common_mask(H):
    """The candidates that share the most frequent histogram.  Half of a rectangle plane's pool are one-pixel regions, whose tile is constant:
    they all get the same answer, so the shares below are set on the others."""
    key = H @ np.random.default_rng(0).random(H.shape[1])          # (equal rows give equal keys; unequal ones practically never do)
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    return inv.reshape(-1) == int(cnt.argmax())


def tune_stage_thresholds(c: Cascade, H, alive, keep, redraw=None, judge=None):
    """Whole-number stage thresholds such that about `keep` of the candidates still alive (the common histogram aside) pass each stage, and
    -- wherever the stage's sums allow it -- at least one is rejected and one passes.  redraw(s) returns new rows for stage s: a short stage
    whose stumps cannot split the candidates anywhere near `keep` is drawn again.  Returns the candidates alive at the end."""
    alive = alive.copy()
    judge = ~common_mask(H) if judge is None else judge
    starts = np.concatenate([[0], np.cumsum(c.stage_n)]).astype(int)
    for s, n in enumerate(c.stage_n):
        if n == 0:
            c.stage_thr[s] = "0"                                       # an empty stage sums to 0: it passes everything or nothing
            continue

        def best_threshold():
            sums = Cascade(c.real, [n], ["0"], c.rows[starts[s]:starts[s] + n]).stage_sums(H)[:, 0]
            v = sums[alive & judge] if (alive & judge).any() else sums[alive]
            if len(v) == 0:
                return (1, 1.0), 0, sums
            best = None
            for t in range(int(np.floor(v.min())), int(np.ceil(v.max())) + 2):
                p = float((v >= t).mean())
                score = (0 if 0 < p < 1 else 1, abs(p - keep))
                if best is None or score < best[0]:
                    best = (score, t)
            return best[0], best[1], sums

        score, t, sums = best_threshold()
        tries = 0
        while redraw is not None and score > (0, 0.15) and tries < 60:
            old = c.rows[starts[s]:starts[s] + n]
            c.rows[starts[s]:starts[s] + n] = redraw(s)
            score2, t2, sums2 = best_threshold()
            if score2 < score:
                score, t, sums = score2, t2, sums2
            else:
                c.rows[starts[s]:starts[s] + n] = old
            tries += 1
        c.stage_thr[s] = str(t)
        alive &= sums >= t
    return alive


def tune_pair(strong: Cascade, weak: Cascade, H, strong_share=0.3, weak_share=0.45, redraw_strong=None, redraw_weak=None, judge=None):
    """Both cascades on one set of candidates: about strong_share end as cls 1, weak_share of the rest as cls 2."""
    ns = max(1, sum(1 for n in strong.stage_n if n > 0))
    nw = max(1, sum(1 for n in weak.stage_n if n > 0))
    passed = tune_stage_thresholds(strong, H, np.ones(len(H), bool), strong_share ** (1.0 / ns), redraw_strong, judge)
    tune_stage_thresholds(weak, H, ~passed, weak_share ** (1.0 / nw), redraw_weak, judge)
    return strong, weak


def report(H, strong: Cascade, weak: Cascade):
    """Shares of cls 0, 1, 2 and the number of rejections per strong / weak stage."""
    cls, _, _, st_s, st_w = classify_model(H, strong, weak)
    shares = [float((cls == k).mean()) for k in (0, 1, 2)]
    rs = [int((st_s == s).sum()) for s in range(len(strong.stage_n))]
    rw = [int((st_w == s).sum()) for s in range(len(weak.stage_n))]
    return shares, rs, rw


# ---- planes -----------------------------------------------------------------------------------------------------------------------------
WANTED_SIZES = [(26, 26), (25, 26),                                    # copy
                (52, 52), (48, 52),                                    # exact 2 x
                (50, 52),                                              # exact 2 x as well: its tile is 25 x 26
                (27, 26), (26, 27), (51, 26), (103, 52), (49, 52),     # one off each special case
                (3, 3), (1, 1), (9, 9),                                # upscale, x clamp
                (12, 100), (5, 40), (2, 19), (1, 9), (19, 10)]         # aspect near both NMS bounds (0.10 < w / h < 2.0)


class _Shelf:
    def __init__(self, x0, y0, x1, y1, gap=3):
        self.x0, self.y0, self.x1, self.y1, self.gap = x0, y0, x1, y1, gap
        self.x, self.y, self.rowh = x0, y0, 0

    def put(self, w, h):
        if self.x + w > self.x1:
            self.x, self.y, self.rowh = self.x0, self.y + self.rowh + self.gap, 0
        if self.y + h > self.y1 or self.x + w > self.x1:
            return None
        at = (self.x, self.y)
        self.x += w + self.gap
        self.rowh = max(self.rowh, h)
        return at


def rect_plane(seed=1, rows=RECT_H, cols=RECT_W):
    """A plane of 200 with dark rectangles whose pixels are uniform in [40, 48) -- one level at thresh_step 8, so a rectangle is one region
    with its exact box, and its texture is what the resize and the LBP see.  Returns (plane, textured boxes, constant boxes, border boxes,
    one-pixel-off boxes): constant SQUARES give code 0 in all 576 pixels (144 in bins 0, 256, 512, 768; a constant oblong's tile has its zero margins); a constant 26 x 26 rectangle with
    the pixel (row 0, column 2) raised gives 143 in bin 0 (that pixel is the v0 neighbour of the first LBP centre alone)."""
    rng = np.random.default_rng(seed)
    img = np.full((rows, cols), 200, np.uint8)
    shelf = _Shelf(24, 24, cols - 24, rows - 24)
    textured, const, border, off1 = [], [], [], []

    def fill(x, y, w, h, value=None):
        # thresh_step 8 puts 40 .. 43 on one level and 44 .. 47 on the next (that is where the tiny regions come from: clusters of the lower
        # one).  A cluster whose box covers more than overlap_coef of the rectangle's would take its place in the pool, so the outermost ring
        # stays on the lower level: the cluster that holds the ring has the exact box too.
        a = rng.integers(40, 48, (h, w))
        ring = np.ones((h, w), bool)
        ring[1:-1, 1:-1] = False
        a[ring] = rng.integers(40, 44, int(ring.sum()))
        img[y:y + h, x:x + w] = a if value is None else value

    for (w, h) in WANTED_SIZES:
        x, y = shelf.put(w, h)
        fill(x, y, w, h)
        textured.append((x, y, w, h))
    for (w, h, v) in ((26, 26, 40), (52, 52, 44), (9, 9, 45), (30, 40, 47), (13, 26, 41)):
        x, y = shelf.put(w, h)
        fill(x, y, w, h, v)
        const.append((x, y, w, h))
    for (px, py) in ((2, 0), (3, 0), (25, 25)):              # (25, 25): the last tile pixel is nobody's neighbour -- still 144
        x, y = shelf.put(26, 26)
        fill(x, y, 26, 26, 40)
        img[y + py, x + px] = 47
        off1.append((x, y, 26, 26))
    while True:                                               # more textured boxes of assorted sizes inside NMS's aspect bounds
        h = int(rng.integers(6, 30))
        w = int(rng.integers(max(1, h // 8 + 1), min(2 * h, 40)))
        at = shelf.put(w, h)
        if at is None:
            break
        fill(at[0], at[1], w, h)
        textured.append((at[0], at[1], w, h))
    # rectangles on each border, the plane's last column and last row among them, and the four corners
    for (x, y, w, h) in ((0, 60, 14, 20), (cols - 14, 100, 14, 20), (100, 0, 20, 15), (200, rows - 15, 20, 15),
                         (0, 0, 12, 12), (cols - 9, 0, 9, 13), (0, rows - 11, 16, 11), (cols - 17, rows - 19, 17, 19)):
        fill(x, y, w, h)
        border.append((x, y, w, h))
    return img, textured, const, border, off1


def pool_of(oracle, plane, prm=RECT_PRM):
    """(boxes (n, 4) xywh in the oracle's pool order, ambiguous count)"""
    ref = oracle.detect_plane(plane, None, None, **prm)
    nd = ref["tree"].nodes[ref["pool"]]
    boxes = np.stack([nd["x"], nd["y"], nd["w"], nd["h"]], axis=1).astype(np.int32) if len(nd) else np.zeros((0, 4), np.int32)
    return boxes, ref["ambiguous"]


def histograms(oracle, plane, boxes):
    H = np.zeros((len(boxes), 1024))
    for i, (x, y, w, h) in enumerate(boxes):
        H[i] = oracle.lbp_hist(plane[y:y + h, x:x + w])
    return H


def pool_histograms(oracle, planes, prm=RECT_PRM):
    """Histograms of every pooled candidate of every plane, one row each."""
    out = []
    for p in planes:
        boxes, _ = pool_of(oracle, p, prm)
        out.append(histograms(oracle, p, boxes))
    return np.concatenate(out) if out else np.zeros((0, 1024))


def count_plane(oracle, n, seed=0, rows=96, cols=128, prm=RECT_PRM):
    """A plane whose pool holds exactly n candidates: textured patches while they fit under n (a patch brings its tiny regions along), then
    single dark pixels, one candidate each."""
    rng = np.random.default_rng(1000 + seed + n)
    img = np.full((rows, cols), 200, np.uint8)
    shelf = _Shelf(2, 2, cols - 2, rows - 2, gap=2)

    def pool_n(a):
        return len(pool_of(oracle, a, prm)[0])

    have = 0
    for _ in range(400):
        if have == n:
            break
        room = n - have
        s = 1 if room < 6 else int(rng.integers(3, 7 if room < 30 else 12))
        h, w = s, max(1, s - int(rng.integers(0, 2)))
        at = shelf.put(w, h)
        assert at is not None, "count_plane: the plane is full"
        trial = img.copy()
        trial[at[1]:at[1] + h, at[0]:at[0] + w] = rng.integers(40, 48, (h, w))
        got = pool_n(trial)
        if got <= n:
            img, have = trial, got
    assert have == n, (have, n)
    return img


def noise_plane(rows, cols, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)


# ---- cascade families: every one is built for both cascades of a context, on the histograms H of the candidates it is run on ----------------
def _table_rows(rng, H, real, dirs):
    """Every listed threshold on each of the four constant-tile dims and on two textured ones, in shuffled order."""
    ud = useful_dims(H, 8)
    dims = list(CONST_DIMS) + [int(d) for d in ud[rng.choice(len(ud), 2, replace=False)]]
    rows = []
    for t in threshold_tokens():
        for d in dims:
            for dr in dirs:
                if real:
                    cp, cn = _pair(rng)
                    rows.append((float(rng.normal()), d, t, cp, cn))
                else:
                    rows.append((float(rng.uniform(0.3, 3.0)), d, dr, t))
    order = rng.permutation(len(rows))
    return [rows[i] for i in order]


def _split(n, k):
    """n stumps in k stages of nearly equal length"""
    return [n // k + (1 if i < n % k else 0) for i in range(k)]


def family_table(H, real, seed=11):
    """The integer table's entries.  REAL: dir +1 only (mode 0).  DISCRETE: every threshold with dir +1 and with dir -1 (modes 0 and 1).
    4 + 4 stages: par."""
    rng = np.random.default_rng(seed + (0 if real else 1))
    out = []
    for _ in range(2):
        rows = _table_rows(rng, H, real, (1,) if real else (1, -1))
        out.append(Cascade(real, _split(len(rows), 4), ["0"] * 4, rows))
    return tune_pair(out[0], out[1], H)


UPPER_COUNT = 142           # a candidate is "upper" when bin 0 holds 142, 143 or 144: the constant tiles and those one or two pixels off


def upper_mask(H):
    return H[:, 0] >= UPPER_COUNT


def family_tablesum(H, real, seed=13):
    """The integer table's entries where every stump's decision reaches a score: 1 + 1 stages, so a score is the sum of ALL rows, and a bias
    stump on bin 0 (threshold 141.5, output +-1000) decides where the upper candidates go.  REAL (dir +1, mode 0): they pass the strong
    cascade, score_strong shows their entries.  DISCRETE (dirs +1 and -1, modes 0 and 1): the strong bias rejects them, the weak bias accepts
    them, score_weak shows their entries.  The stage thresholds are tuned on the other candidates alone.  par (2 stages)."""
    rng = np.random.default_rng(seed + (0 if real else 1))
    dirs = (1,) if real else (1, -1)
    rs, rw = _table_rows(rng, H, real, dirs), _table_rows(rng, H, real, dirs)
    if real:
        rs = [(1.0, 0, "141.5", 0.0, 1000.0)] + rs
    else:
        rs = [(1000.0, 0, 1, "141.5")] + rs
        rw = [(1000.0, 0, -1, "141.5")] + rw
    s, w = Cascade(real, [len(rs)], ["0"], rs), Cascade(real, [len(rw)], ["0"], rw)
    return tune_pair(s, w, H, strong_share=0.3 if real else 0.5, weak_share=0.45 if real else 0.3, judge=~upper_mask(H))


def swap_token(c: Cascade, a, b, dr):
    """c with threshold token a replaced by b in the rows of direction dr (REAL rows have dir +1)"""
    if c.real:
        rows = [(w, d, b if t == a else t, cp, cn) for (w, d, t, cp, cn) in c.rows] if dr == 1 else c.rows
    else:
        rows = [(w, d, r, b if (t == a and r == dr) else t) for (w, d, r, t) in c.rows]
    return Cascade(c.real, c.stage_n, c.stage_thr, rows)


PATH_STRONG, PATH_WEAK = 2400, 2376            # 4776 = CLS_AB_CAP stumps together


def path_rows(H, seed=21):
    """The rows every path-selection shape shares: DISCRETE with dirs +1 and -1, 2400 strong and 2377 weak (the last weak row is only part
    of the 4777-stump shape)."""
    rng = np.random.default_rng(seed)
    return random_rows(rng, H, PATH_STRONG, False), random_rows(rng, H, PATH_WEAK + 1, False)


def family_path(H, shape, seed=21):
    """shape: "8+8" (par), "9+8" and "16+1" (lane_cascade_fast), "4777" (8 + 8 stages, one stump over CLS_AB_CAP: generic with unit dirs),
    "dir2" (one strong stump with dir 2: generic, modes 0, 1 and 2), "odd" (dirs from {0, 2, -3}, NaN and infinite thresholds mixed in)."""
    rs, rw = path_rows(H, seed)
    ks, kw = {"9+8": (9, 8), "16+1": (16, 1)}.get(shape, (8, 8))
    if shape != "4777":
        rw = rw[:PATH_WEAK]
    if shape == "dir2":
        w, d, _, t = rs[1000]
        rs = rs[:1000] + [(w, d, 2, t)] + rs[1001:]
    if shape == "odd":
        rng = np.random.default_rng(seed + 1)
        rs = random_rows(rng, H, 300, False, dirs=(0, 2, -3, 2, -3), thr_tokens=["nan", "inf", "-inf", "-0.0"])
        rw = random_rows(rng, H, 260, False, dirs=(0, 2, -3, 2, -3), thr_tokens=["nan", "inf", "-inf", "-0.0"])
    s = Cascade(False, _split(len(rs), ks), ["0"] * ks, rs)
    w = Cascade(False, _split(len(rw), kw), ["0"] * kw, rw)
    return tune_pair(s, w, H)


STAGE_LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200]


def family_lengths(H, long_is, form, seed=31):
    """The stage loops' block sizes: the twelve lengths as the strong (long_is = 0) or the weak (1) cascade, the other one short.
    form "par": 12 + 4 stages; "fast": 12 + 5 (17 stages: lane_cascade_fast); "generic": 12 + 4 with one dir-2 stump in the short cascade.
    The weak file holds 37 rows more than num_of_iter announces."""
    rng = np.random.default_rng(seed + long_is)
    short_n = [5, 3, 11, 2] + ([6] if form == "fast" else [])
    long_rows = random_rows(rng, H, sum(STAGE_LENGTHS), False)
    short_rows = random_rows(rng, H, sum(short_n), False)
    if form == "generic":
        w, d, _, t = short_rows[4]
        short_rows[4] = (w, d, 2, t)
    long_c = Cascade(False, STAGE_LENGTHS, ["0"] * len(STAGE_LENGTHS), long_rows)
    short_c = Cascade(False, short_n, ["0"] * len(short_n), short_rows)
    s, w = (long_c, short_c) if long_is == 0 else (short_c, long_c)
    fixed = {id(short_c): {0}} if form == "generic" else {}          # (the stage that holds the dir-2 stump is not drawn again)

    def redraw(c):
        def rows_of(k):
            at = sum(c.stage_n[:k])
            if c.stage_n[k] > 11 or k in fixed.get(id(c), ()):
                return c.rows[at:at + c.stage_n[k]]
            return random_rows(rng, H, c.stage_n[k], False)
        return rows_of

    tune_pair(s, w, H, redraw_strong=redraw(s), redraw_weak=redraw(w))
    w.rows = w.rows + random_rows(rng, H, 37, False)
    return s, w


TRUNC_TOKENS = ["-0.7", "1.9", "-1.9", "0"]
# sums that the (int) truncation decides differently from the number as written: -0.7 -> 0 rejects (-0.7, 0), 1.9 -> 1 passes [1, 1.9),
# -1.9 -> -1 rejects [-1.9, -1); "0" has no such interval
TRUNC_BETWEEN = [(-0.7, 0.0), (1.0, 1.9), (-1.9, -1.0), None]


def family_trunc(H, seed=41):
    """Stage thresholds written as -0.7, 1.9, -1.9, 0 (REAL, 4 + 4 stages, par).  The thresholds are fixed, so each stage starts with a
    bias stump (threshold inf: always cp) that moves the stage's sums until about the wanted share passes; the other outputs are small, so
    sums fall between the truncated and the written value."""
    rng = np.random.default_rng(seed)
    out = []
    alive = np.ones(len(H), bool)
    judge = ~common_mask(H)
    for which in range(2):
        n = [24, 25, 23, 26]
        rows = []
        for k in n:
            rows.append((1.0, 0, "inf", 0.0, 0.0))
            for (w, d, t, cp, cn) in random_rows(rng, H, k - 1, True):
                rows.append((w, d, t, cp * 0.15, cn * 0.15))
        c = Cascade(True, n, TRUNC_TOKENS, rows)
        keep = (0.3 if which == 0 else 0.45) ** 0.25
        off = 0
        for s, k in enumerate(n):
            sums = c.stage_sums(H)[:, s]
            q = float(np.quantile(sums[alive & judge], 1.0 - keep)) if (alive & judge).any() else 0.0
            target = int(float(TRUNC_TOKENS[s]))
            w, d, t, _, cn = c.rows[off]
            c.rows[off] = (w, d, t, round(target - q + 0.0006, 3), cn)
            alive = alive & (c.stage_sums(H)[:, s] >= int(float(TRUNC_TOKENS[s])))
            off += k
        out.append(c)
        alive = ~alive if which == 0 else alive
    return out[0], out[1]


CHUNK_STRONG, CHUNK_WEAK = [1023, 1024, 1025], [2048, 2049]


def family_chunks(H, seed=51):
    """Stage lengths around CLS_CHUNK = 1024 of block_cascade and k_cascade_fv (REAL rows with fractional thresholds).  7169 stumps: k_classify
    takes lane_cascade_generic on them."""
    rng = np.random.default_rng(seed)
    s = Cascade(True, CHUNK_STRONG, ["0"] * 3, random_rows(rng, H, sum(CHUNK_STRONG), True))
    w = Cascade(True, CHUNK_WEAK, ["0"] * 2, random_rows(rng, H, sum(CHUNK_WEAK), True))
    return tune_pair(s, w, H)


SMALL_STRONG, SMALL_WEAK = [70, 64, 30, 65, 8, 130], [64, 9, 100, 63, 20]


def family_small(H, form, seed=61):
    """A cascade pair small enough for pools of thousands of candidates and batches of many planes: DISCRETE, dirs +1 and -1, 6 + 5 stages
    of 367 + 256 stumps.  form "par": the stage-parallel path; "generic": one strong stump has dir 2, so all_unit is off."""
    rng = np.random.default_rng(seed)
    rs, rw = random_rows(rng, H, sum(SMALL_STRONG), False), random_rows(rng, H, sum(SMALL_WEAK), False)
    if form == "generic":
        w, d, _, t = rs[100]
        rs[100] = (w, d, 2, t)
    return tune_pair(Cascade(False, SMALL_STRONG, ["0"] * 6, rs), Cascade(False, SMALL_WEAK, ["0"] * 5, rw), H)


def small_plane(seed, rows=64, cols=64):
    """A plane of 200 with a few textured rectangles, like rect_plane but of any size"""
    rng = np.random.default_rng(seed)
    img = np.full((rows, cols), 200, np.uint8)
    shelf = _Shelf(1, 1, cols - 1, rows - 1, gap=2)
    while True:
        h = int(rng.integers(3, 24))
        w = int(rng.integers(max(1, h // 8 + 1), min(2 * h, 30)))
        at = shelf.put(w, h)
        if at is None:
            return img
        img[at[1]:at[1] + h, at[0]:at[0] + w] = rng.integers(40, 48, (h, w))


NOISE_ROWS, NOISE_COLS = 128, 185


def special_feature_rows(H, seed=71):
    """Feature vectors for CascadeBoost::predict on its own: histogram rows as they are, then rows moved off the integers, negated, and with
    1e300, -1e300, NaN and the infinities put into a tenth of the bins each."""
    rng = np.random.default_rng(seed)
    base = H[rng.choice(len(H), 60, replace=len(H) < 60)]
    out = [base, base + 0.5, base - 0.25, -base, base * 1.0000001]
    for v in (1e300, -1e300, np.nan, np.inf, -np.inf):
        a = base.copy()
        a[rng.random(a.shape) < 0.1] = v
        out.append(a)
    return np.concatenate(out)
