"""The numpy reference of the splitting of touching glyphs (str_er_feet_split, str_er_split_words): the contract at str_er_run_split
(include/str_er.h).  Profiles, cuts and pieces come from boolean footprints, piece tiles go through run_read_ref.py, and the
segmentation of a run is a brute force over all compositions of its atoms.  It shares no code with the library."""
import itertools

import numpy as np

import line_words_ref as LW
import run_read_ref as RR

MAX_W = 1024


def threshold(H, num=1, den=4):
    return H * num // den                                      # (Python integers: exact)


def valleys(n, thr):
    """[(d, p, a, b)] of a column profile: the maximal intervals [a, b) with n <= thr that touch neither end, with their depth and
    cut column."""
    n = [int(v) for v in n]
    W, out, c = len(n), [], 0
    while c < W:
        if n[c] > thr:
            c += 1
            continue
        a = c
        while c < W and n[c] <= thr:
            c += 1
        if a == 0 or c == W:
            continue
        d = min(n[a:c])
        at = [k for k in range(a, c) if n[k] == d]
        out.append((d, (at[0] + at[-1]) // 2, a, c))
    return out


def cuts(n, H, num=1, den=4):
    """(the kept cut columns of a profile, ascending; thr)."""
    thr = threshold(H, num, den)
    if len(n) > MAX_W:
        return [], thr
    v = sorted((d, p) for d, p, _, _ in valleys(n, thr))[:3]
    return sorted(p for _, p in v), thr


def piece_nodes(A):
    """The pieces (i, j) of a run of A atoms, in order; none for an uncut run."""
    return [(i, j) for i in range(A) for j in range(i + 1, A + 1) if (i, j) != (0, A)] if A > 1 else []


def tables(feet, num=1, den=4, gap_num=1, gap_den=3):
    """(the three tables of line_words_ref.tables; splits: (n_cuts, cut0, cut1, cut2, thr, first_piece, n_pieces, 0) per run; pieces:
    (run, from, to, x0, x1, y0, y1, pixels); the line of every run) of footprints [(x, y, bits), ...]."""
    tabs = LW.tables(feet, gap_num, gap_den)
    splits, pieces, line_of = [], [], []
    for t, (x, y, bits) in enumerate(feet):
        bits = np.asarray(bits, bool)
        lw = tabs[0][t]
        for r in range(lw[2], lw[2] + lw[3]):
            x0, x1, y0, y1 = tabs[1][r][:4]
            box = bits[y0 - y:y1 - y, x0 - x:x1 - x]
            n = box.sum(axis=0)
            assert (n >= 1).all()
            cs, thr = cuts(n, y1 - y0, num, den)
            node = [0] + cs + [x1 - x0]
            pn = piece_nodes(len(cs) + 1)
            splits.append((len(cs), *[x0 + c for c in cs], *([-1] * (3 - len(cs))), thr, len(pieces), len(pn), 0))
            for i, j in pn:
                sub = box[:, node[i]:node[j]]
                rows = np.flatnonzero(sub.any(axis=1))
                pieces.append((r, i, j, x0 + node[i], x0 + node[j], y0 + int(rows[0]), y0 + int(rows[-1]) + 1, int(sub.sum())))
            line_of.append(t)
    return tabs, splits, pieces, line_of


def piece_tiles(feet, pieces, line_of):
    """The tile of every piece: the rule of a run's tile on the piece's box."""
    out = []
    for p in pieces:
        x, y, bits = feet[line_of[p[0]]]
        out.append(RR.tile_of(np.asarray(bits, bool), x, y, p[3:7]))
    return out


def piece_features(oracle, feet, pieces, line_of, slopes=None):
    tl = piece_tiles(feet, pieces, line_of)
    q = np.zeros((len(tl), 1800), np.uint8)
    for k, (tile, p) in enumerate(zip(tl, pieces)):
        q[k] = oracle.chain_features(tile, RR.slope_of(slopes[line_of[p[0]]]) if slopes is not None else 0.0)
    return q, tl


def as_lists(splits, pieces):
    """Record arrays of the binding as the lists of tuples `tables` returns."""
    return ([(int(s["n_cuts"]), *[int(v) for v in s["cut"]], int(s["thr"]), int(s["first_piece"]), int(s["n_pieces"]), int(s["n_parts"])) for s in splits],
            [tuple(int(v) for v in p) for p in pieces.tolist()])


# ---- the segmentation ------------------------------------------------------------------------------------------------------------------

def compositions(A):
    """Every way to write the atoms 0 .. A-1 as consecutive pieces: lists of (i, j), ordered so that the first minimum is the one the
    recurrence's tie rule picks (see segment_brute)."""
    out = []
    for k in range(A):
        for inner in itertools.combinations(range(1, A), k):
            node = [0, *inner, A]
            out.append(list(zip(node[:-1], node[1:])))
    return out


def segment_brute(m, A, split):
    """(cost, parts) of a run: the minimum over all compositions (at most 8) of the sum of m[(i, j)] plus `split` per part after the
    first.  Among the compositions of minimal cost the recurrence takes, from the run's end backwards, the part with the smallest
    start: the one whose list of starts, read from the end, is smallest."""
    best = None
    for comp in compositions(A):
        cost = sum(m[p] for p in comp) + split * (len(comp) - 1)
        key = (cost, [i for i, _ in reversed(comp)])
        if best is None or key < best[0]:
            best = (key, comp)
    return best[0][0], best[1]


def segment_dp(m, A, split):
    """The recurrence of the contract as it is written."""
    D, pred = [0], [0]
    for j in range(1, A + 1):
        c = [D[i] + m[(i, j)] + (split if i > 0 else 0) for i in range(j)]
        D.append(min(c))
        pred.append(c.index(min(c)))
    parts, j = [], A
    while j > 0:
        parts.append((pred[j], j))
        j = pred[j]
    return D[A], parts[::-1]


def split_words(splits, run_costs, piece_costs, first_run, n_of, split=8):
    """(word splits (first_part, n_parts, cost, read_cost), parts (run, piece), the parts' rows) by brute force."""
    rc, pc = np.asarray(run_costs, np.uint8).reshape(-1, 65), np.asarray(piece_costs, np.uint8).reshape(-1, 65)
    words, parts, rows = [], [], []
    for f, k in zip(first_run, n_of):
        first, cost, read = len(parts), 0, 0
        for r in range(f, f + k):
            A, fp = splits[r][0] + 1, splits[r][5]
            pn = piece_nodes(A)
            m = {p: int(pc[fp + i].min()) for i, p in enumerate(pn)}
            m[(0, A)] = int(rc[r].min())
            c, comp = segment_brute(m, A, split)
            cost += c
            read += m[(0, A)]
            for p in comp:
                piece = -1 if p == (0, A) else fp + pn.index(p)
                parts.append((r, piece))
                rows.append(rc[r] if piece < 0 else pc[piece])
        words.append((first, len(parts) - first, cost, read))
    return words, parts, np.array(rows, np.uint8).reshape(-1, 65)


def split_text(parts, rows):
    """The characters of parts: the first arg min of every row."""
    return [RR.ocr_char(int(np.argmin(r))) for r in rows]


# ---- a model that knows given tiles -----------------------------------------------------------------------------------------------------

def prototype_model(q, gamma=0.2, slope=12.0):
    """A libsvm text model (c_svc, rbf, 65 classes with the labels 0 .. 64, probability outputs) with one support vector a class: the
    feature rows q[c] (8-bit numerators over 255), class c = row c; fewer than 65 rows are repeated.  The decision value of the pair
    (i, j) is K(x, q[i]) - K(x, q[j]) and its sigmoid has the slope `slope`: a tile that is one of the rows is read as its class with a
    high probability, a tile far from every row gets 1 / 65 a class.  The values are exact k / 255 doubles (the loader's byte form)."""
    q = np.asarray(q, np.uint8)
    assert q.ndim == 2 and len(q) >= 1
    k = 65
    rows = q[np.arange(k) % len(q)]
    npairs = k * (k - 1) // 2
    f = lambda v: "%.17g" % v
    out = ["svm_type c_svc", "kernel_type rbf", "gamma " + f(gamma), f"nr_class {k}", f"total_sv {k}", "rho " + " ".join(["0"] * npairs),
           "label " + " ".join(str(i) for i in range(k)), "probA " + " ".join([f(-slope)] * npairs), "probB " + " ".join(["0"] * npairs),
           "nr_sv " + " ".join(["1"] * k), "SV"]
    for c in range(k):
        # (libsvm: the vector of class c carries, for the other class j, its coefficient at j - 1 if j > c -- it is the pair's first class -- else at j)
        co = " ".join("1" if j >= c else "-1" for j in range(k - 1))
        feats = " ".join(f"{j}:{f(int(v) / 255.0)}" for j, v in enumerate(rows[c]) if v)          # (index j: feature j, as the shipped models count)
        out.append(co + " " + feats + " ")
    return ("\n".join(out) + "\n").encode()
