"""Reference of the str_er_shape contract (include/str_er.h) in numpy / scipy, for the shape tests.  Not a test module."""
import numpy as np
from scipy import ndimage

FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
EIGHT = np.ones((3, 3), int)


def _hull_area2(mask):
    """Twice the area of the convex hull of the corners of the pixel squares of mask, by a monotone chain and the shoelace formula."""
    pts = set()
    for y in range(mask.shape[0]):
        xs = np.nonzero(mask[y])[0]
        if len(xs):
            for x in (int(xs[0]), int(xs[-1]) + 1):
                pts.add((x, y))
                pts.add((x, y + 1))
    pts = sorted(pts)
    if len(pts) < 3:
        return 0

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    hull = lower[:-1] + upper[:-1]
    return abs(sum(hull[i][0] * hull[(i + 1) % len(hull)][1] - hull[(i + 1) % len(hull)][0] * hull[i][1] for i in range(len(hull))))


def holes(mask):
    """The holes of mask: 8-connected components of the complement that do not reach outside the box (a ring of non-mask
    pixels around it).  Returns (count, pixels)."""
    h, w = mask.shape
    out = np.ones((h + 2, w + 2), bool)
    out[1:-1, 1:-1] = ~mask
    lab, n = ndimage.label(out, structure=EIGHT)
    outside = lab[0, 0]
    inner = (lab != 0) & (lab != outside)
    return len(set(np.unique(lab[inner]).tolist())), int(inner.sum())


def shape_ref(mask, plane_box):
    """The str_er_shape fields of a bool mask (h, w) over its box, with plane_box = P' (uint8, the same shape) under the box."""
    m = np.asarray(mask, bool)
    h, w = m.shape
    p = np.asarray(plane_box).astype(np.int64)
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = m
    c = pad[1:-1, 1:-1]
    perimeter = int(sum((c & ~pad[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]).sum() for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0))))
    _, n4 = ndimage.label(m, structure=FOUR)
    n_holes, hole_pixels = holes(m)
    cr = []
    for j in (1, 3, 5):
        row = np.concatenate([[False], m[j * h // 6], [False]])
        cr.append(int((row[1:] != row[:-1]).sum()))
    return {"pixels": int(m.sum()), "perimeter": perimeter, "euler": int(n4) - n_holes, "hole_pixels": hole_pixels,
            "crossings": cr + [sorted(cr)[1]], "hull_area2": _hull_area2(m), "grey_sum": int(p[m].sum()), "grey_sum2": int((p[m] ** 2).sum())}


def as_dict(rec):
    """One SHAPE_DTYPE record as shape_ref's dict."""
    return {"pixels": int(rec["pixels"]), "perimeter": int(rec["perimeter"]), "euler": int(rec["euler"]), "hole_pixels": int(rec["hole_pixels"]),
            "crossings": [int(v) for v in rec["crossings"]], "hull_area2": int(rec["hull_area2"]), "grey_sum": int(rec["grey_sum"]),
            "grey_sum2": int(rec["grey_sum2"])}
