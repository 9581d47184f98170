"""Reference of the str_er_stroke contract (include/str_er.h) in numpy / scipy, for the stroke tests.  Not a test module.

E_0 = M; E_k = E_{k-1} eroded through N_k (4-neighbours for odd k, 8-neighbours for even k), with everything outside the box outside
every E_k; D(p) = k for p in E_{k-1} minus E_k; the ridge is the pixels of M whose 8 neighbours all have D <= D(p) (D = 0 outside M)."""
import numpy as np
from scipy import ndimage

FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
EIGHT = np.ones((3, 3), bool)
FIELDS = ("depth_max", "ridge_pixels", "depth_sum", "ridge_depth_sum", "ridge_depth_sum2")


def erosions(mask):
    """[E_0, E_1, ..., E_K] of a bool mask (E_K is the first empty one)."""
    e = [np.asarray(mask, bool).copy()]
    while e[-1].any():
        k = len(e)
        e.append(ndimage.binary_erosion(e[-1], structure=FOUR if k % 2 else EIGHT, border_value=0))
    return e


def depth(mask):
    """D of every pixel of the box (0 outside M).  Each erosion runs on the bounding box of E_{k-1} only: outside it E_{k-1} is empty,
    which is what border_value=0 assumes, so the result is the same and a large region costs its shrinking boxes, not K full boxes."""
    e = np.asarray(mask, bool).copy()
    d = np.zeros(e.shape, np.int64)
    k = 0
    while e.any():
        k += 1
        ys, xs = np.nonzero(e)
        win = (slice(ys.min(), ys.max() + 1), slice(xs.min(), xs.max() + 1))
        sub = e[win]
        nxt = ndimage.binary_erosion(sub, structure=FOUR if k % 2 else EIGHT, border_value=0)
        d[win][sub & ~nxt] = k
        e[win] = nxt
    return d


def ridge(mask):
    """The ridge by the local-maximum rule: maximum_filter over the 8-neighbourhood, outside the box 0."""
    m = np.asarray(mask, bool)
    d = depth(m)
    return m & (d >= ndimage.maximum_filter(d, footprint=EIGHT, mode="constant", cval=0))


def ridge_bitrows(mask):
    """The ridge by the kernels' bit-row form: the union over k of (E_{k-1} & ~E_k) & ~dilate8(E_k)."""
    e = erosions(mask)
    r = np.zeros(np.shape(mask), bool)
    for k in range(1, len(e)):
        r |= e[k - 1] & ~e[k] & ~ndimage.binary_dilation(e[k], structure=EIGHT)
    return r


def stroke_ref(mask):
    """The str_er_stroke fields of a bool mask (h, w) over its box, as a dict."""
    m = np.asarray(mask, bool)
    d = depth(m)
    r = m & (d >= ndimage.maximum_filter(d, footprint=EIGHT, mode="constant", cval=0))
    rd = d[r]
    return {"depth_max": int(d.max()), "ridge_pixels": int(r.sum()), "depth_sum": int(d[m].sum()), "ridge_depth_sum": int(rd.sum()),
            "ridge_depth_sum2": int((rd * rd).sum())}


def as_dict(rec):
    """One STROKE_DTYPE record as stroke_ref's dict."""
    return {k: int(rec[k]) for k in FIELDS}
