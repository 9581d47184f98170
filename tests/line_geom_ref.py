"""The reference of the line geometry (STR_ER_WANT_LINE_GEOM, str_er_feet_geom, str_er_hull_of_points, str_er_quad_from_hull): the
contract at str_er_line_geom (include/str_er.h) in Python integers and fractions.Fraction.  The hull is found by gift wrapping over
every corner of every pixel square -- neither the row-extent chains of the kernel nor the sorted chain of the host function."""
from fractions import Fraction

import numpy as np

FIELDS = ("hull_area2", "m10", "m01", "m20", "m11", "m02", "pixels", "edge", "ex", "ey", "dmin", "dmax", "cmin", "cmax")


def hull_of_points(points):
    """The strictly convex hull of integer points as a list of (x, y), clockwise on screen (x right, y down) from the smallest (y, x).
    One point gives one vertex, collinear points their two ends."""
    pts = np.unique(np.asarray(points, np.int64).reshape(-1, 2), axis=0)
    if len(pts) == 0:
        return []
    start = pts[np.lexsort((pts[:, 0], pts[:, 1]))[0]]
    out = [(int(start[0]), int(start[1]))]
    p = start
    while True:
        v = pts - p
        rest = np.nonzero((v != 0).any(axis=1))[0]
        if len(rest) == 0:
            break
        q = rest[0]
        while True:               # until every point lies clockwise of p -> q (turn >= 0)
            turn = v[q, 0] * v[:, 1] - v[q, 1] * v[:, 0]
            k = int(np.argmin(turn))
            if turn[k] >= 0:
                break
            q = k
        on = np.nonzero((turn == 0) & (v[:, 0] * v[q, 0] + v[:, 1] * v[q, 1] > 0))[0]      # collinear ahead: the farthest is the vertex
        q = on[np.argmax(np.abs(v[on]).sum(axis=1))]
        nxt = (int(pts[q, 0]), int(pts[q, 1]))
        if nxt == out[0] or (len(out) >= 2 and nxt == out[-2]):       # closed, or a segment walked back
            break
        out.append(nxt)
        p = pts[q]
    return out


def corners(bits, x0=0, y0=0):
    """Every corner of every pixel square of the boolean array bits whose pixel (0, 0) is the frame pixel (x0, y0)."""
    ys, xs = np.nonzero(bits)
    c = np.concatenate([np.stack([xs + dx, ys + dy], 1) for dx in (0, 1) for dy in (0, 1)]) if len(xs) else np.zeros((0, 2), np.int64)
    return np.unique(c.astype(np.int64) + np.array([x0, y0], np.int64), axis=0)


def moments(bits, x0=0, y0=0):
    ys, xs = np.nonzero(bits)
    xs, ys = [int(x) + x0 for x in xs], [int(y) + y0 for y in ys]
    return dict(pixels=len(xs), m10=sum(xs), m01=sum(ys), m20=sum(x * x for x in xs), m11=sum(x * y for x, y in zip(xs, ys)), m02=sum(y * y for y in ys))


def quad(hull):
    """hull_area2, the chosen edge, its integers and the four corners (as float(Fraction)) of a hull with at least 3 vertices."""
    n = len(hull)
    area2 = sum(hull[i][0] * hull[(i + 1) % n][1] - hull[(i + 1) % n][0] * hull[i][1] for i in range(n))
    best = None
    for i in range(n):
        ex, ey = hull[(i + 1) % n][0] - hull[i][0], hull[(i + 1) % n][1] - hull[i][1]
        d = [x * ex + y * ey for x, y in hull]
        c = [-x * ey + y * ex for x, y in hull]
        den = ex * ex + ey * ey
        a = Fraction((max(d) - min(d)) * (max(c) - min(c)), den)
        if best is None or a < best[0]:
            best = (a, i, ex, ey, min(d), max(d), min(c), max(c), den)
    _, i, ex, ey, d0, d1, c0, c1, den = best
    qx = [float(Fraction(d * ex - c * ey, den)) for d, c in ((d0, c0), (d1, c0), (d1, c1), (d0, c1))]
    qy = [float(Fraction(d * ey + c * ex, den)) for d, c in ((d0, c0), (d1, c0), (d1, c1), (d0, c1))]
    return dict(hull_area2=area2, edge=i, ex=ex, ey=ey, dmin=d0, dmax=d1, cmin=c0, cmax=c1), qx, qy


EMPTY = (dict(hull_area2=0, m10=0, m01=0, m20=0, m11=0, m02=0, pixels=0, edge=-1, ex=0, ey=0, dmin=0, dmax=0, cmin=0, cmax=0), [0.0] * 4, [0.0] * 4, [])


def geom(bits, x0=0, y0=0):
    """(integer fields, qx, qy, hull) of the footprint bits at (x0, y0)."""
    if not np.asarray(bits).any():
        return EMPTY
    hull = hull_of_points(corners(bits, x0, y0))
    ints, qx, qy = quad(hull)
    ints.update(moments(bits, x0, y0))
    return ints, qx, qy, hull


def merged(geoms, rep):
    """A frame line from the references of its members: the hull of the union of their hull vertices, the moments of `rep`."""
    pts = [p for g in geoms for p in g[3]]
    if not pts:
        return EMPTY
    hull = hull_of_points(pts)
    ints, qx, qy = quad(hull)
    ints.update({k: rep[0][k] for k in ("pixels", "m10", "m01", "m20", "m11", "m02")})
    return ints, qx, qy, hull


def same(rec, points, ref):
    """A LINE_GEOM_DTYPE record and the (n, 2) vertex array it indexes against a reference: every field with ==.  Returns a message or None."""
    ints, qx, qy, hull = ref
    for k in FIELDS:
        if int(rec[k]) != ints[k]:
            return f"{k}: {int(rec[k])} != {ints[k]}"
    if int(rec["count"]) != len(hull):
        return f"count: {int(rec['count'])} != {len(hull)}"
    got = [(int(x), int(y)) for x, y in points[int(rec["first"]):int(rec["first"]) + int(rec["count"])]]
    if got != hull:
        return f"hull: {got} != {hull}"
    if [float(v) for v in rec["qx"]] != qx or [float(v) for v in rec["qy"]] != qy:
        return f"corners: {rec['qx']}, {rec['qy']} != {qx}, {qy}"
    return None


# ---- the hand-made footprints both test files use ------------------------------------------------------------------------------------------

FRAME_W, FRAME_H = 1400, 1200


def shapes():
    """{name: (x0, y0, bits)} on a FRAME_W x FRAME_H frame: the smallest footprints at which the kernel or the host functions can go wrong."""
    W, H = FRAME_W, FRAME_H
    one = np.ones((1, 1), bool)
    out = {"pixel_00": (0, 0, one), "pixel_last": (W - 1, H - 1, one)}
    out["row_65"] = (31, 5, np.ones((1, 65), bool))                     # crosses the 32-bit and the 64-bit word borders
    out["column_65"] = (7, 10, np.ones((65, 1), bool))                  # more rows than lanes
    two = np.zeros((10, 70), bool)                                      # two blobs, empty rows between them, rows with bits in the last word only
    two[0, :] = True; two[1, 66:] = True; two[2, 3:41] = True
    two[7, 64:] = True; two[8, 10:21] = True; two[9, :6] = True
    out["two_blobs"] = (33, 40, two)
    out["staircase"] = (200, 20, np.eye(100, dtype=bool))               # collinear corners
    bar = np.zeros((55, 200), bool)                                     # a slanted bar, 6 pixels thick, one pixel down every 4: a rotated box
    for c in range(200):
        bar[c // 4:c // 4 + 6, c] = True
    out["sheared_bar"] = (300, 200, bar)
    yy, xx = np.mgrid[-40:41, -40:41]
    out["disc_40"] = (500, 300, xx * xx + yy * yy <= 1600)
    # the lens: 70 rows, mirrored about the middle; the row at the distance j from the two middle rows ends j (j + 1) / 2 pixels short of
    # theirs on either side, so the steps shrink towards the middle, the outline is convex and every row end is a hull vertex
    half = [k * (k + 1) // 2 for k in range(35)]
    lens = np.zeros((70, 2 * half[-1] + 1), bool)
    for r in range(70):
        j = 34 - r if r < 35 else r - 35
        lens[r, half[j]:2 * half[-1] + 1 - half[j]] = True
    out["lens_70"] = (100, 700, lens)
    tall = np.zeros((1100, 3), bool)                                    # taller than the kernel's LDS rows: the scratch path
    tall[np.arange(1100), (np.arange(1100) // 7) % 3] = True
    out["tall_1100"] = (1300, 50, tall)
    return out


def random_feet(rng, n=200):
    """n footprints, each a union of rectangles in a box of up to 150 x 90 at a random origin (tight boxes); number 17 is empty."""
    out = []
    for i in range(n):
        w, h = int(rng.integers(1, 151)), int(rng.integers(1, 91))
        bits = np.zeros((h, w), bool)
        for _ in range(int(rng.integers(1, 5))):
            x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
            bits[y0:int(rng.integers(y0, h)) + 1, x0:int(rng.integers(x0, w)) + 1] = True
        rows, cols = np.nonzero(bits.any(axis=1))[0], np.nonzero(bits.any(axis=0))[0]
        bits = bits[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1]
        if i == 17:
            bits = np.zeros((0, 0), bool)
        h, w = bits.shape
        out.append((int(rng.integers(0, FRAME_W - w + 1)), int(rng.integers(0, FRAME_H - h + 1)), bits))
    return out
