"""The numpy reference of the frame maps (STR_ER_WANT_TEXT_MAP / _LINE_MAP, str_er_text_map_regions): the pixel rule of
str_er_frame_map in exact integers, a region rasterised with its mask."""
import numpy as np

NO_ID = np.iinfo(np.int64).max


def samples(n_out, n_lvl):
    """xs(x) = ((2x + 1) * n_lvl) // (2 * n_out) for x in [0, n_out): the level sample of every frame coordinate."""
    x = np.arange(n_out, dtype=np.int64)
    return ((2 * x + 1) * int(n_lvl)) // (2 * int(n_out))


class Raster:
    """The byte map (OR of values) and the id map (min of ids, -1 for none) of one W x H frame."""

    def __init__(self, W, H):
        self.W, self.H = int(W), int(H)
        self.map = np.zeros((self.H, self.W), np.uint8)
        self.ids = np.full((self.H, self.W), NO_ID, np.int64)
        self._tab = {}

    def _s(self, n, nl):
        k = (n, int(nl))
        if k not in self._tab:
            self._tab[k] = samples(n, nl)
        return self._tab[k]

    def add(self, pw, ph, x, y, mask, value, ident=None):
        """A region of a plane of level size (pw, ph): box (x, y, w, h) = its mask's shape at (x, y)."""
        h, w = mask.shape
        xs, ys = self._s(self.W, pw), self._s(self.H, ph)
        c0, c1 = np.searchsorted(xs, x, "left"), np.searchsorted(xs, x + w, "left")        # (xs is non-decreasing)
        r0, r1 = np.searchsorted(ys, y, "left"), np.searchsorted(ys, y + h, "left")
        if c0 >= c1 or r0 >= r1:
            return
        sub = mask[np.ix_(ys[r0:r1] - y, xs[c0:c1] - x)]
        if value:
            self.map[r0:r1, c0:c1] |= np.where(sub, np.uint8(value), np.uint8(0))
        if ident is not None:
            blk = self.ids[r0:r1, c0:c1]
            self.ids[r0:r1, c0:c1] = np.where(sub, np.minimum(blk, int(ident)), blk)

    def id_map(self):
        return np.where(self.ids == NO_ID, -1, self.ids).astype(np.int32)


def brute(W, H, regions):
    """The pixel rule pixel by pixel: regions = (pw, ph, x, y, mask, value, id or None)."""
    m = np.zeros((H, W), np.uint8)
    ids = np.full((H, W), -1, np.int64)
    for yy in range(H):
        for xx in range(W):
            for pw, ph, x, y, mask, value, ident in regions:
                xs, ys = ((2 * xx + 1) * pw) // (2 * W), ((2 * yy + 1) * ph) // (2 * H)
                h, w = mask.shape
                if x <= xs < x + w and y <= ys < y + h and mask[ys - y, xs - x]:
                    m[yy, xx] |= value
                    if ident is not None and (ids[yy, xx] < 0 or ident < ids[yy, xx]):
                        ids[yy, xx] = ident
    return m, ids.astype(np.int32)
