"""The numpy reference of the frame lines (STR_ER_WANT_FRAME_LINES, str_er_line_feet_regions, str_er_frame_lines_from_pairs): the
contract at str_er_line_foot (include/str_er.h) in boolean arrays and Python integers."""
import numpy as np

from text_map_ref import samples


class Foot:
    """The footprint of one line: its foot box in frame pixels and the boolean pixels over it (h, w)."""

    def __init__(self, x=0, y=0, bits=None):
        self.bits = np.zeros((0, 0), bool) if bits is None else bits
        self.h, self.w = self.bits.shape
        self.x, self.y = (int(x), int(y)) if self.w else (0, 0)
        self.pixels = int(self.bits.sum())

    def words(self):
        """The str_er_mask layout of the footprint: h rows of (w + 31) // 32 uint32 words."""
        pitch = (self.w + 31) // 32
        pad = np.zeros((self.h, pitch * 32), np.uint8)
        pad[:, :self.w] = self.bits
        return np.packbits(pad, axis=1, bitorder="little").view("<u4").reshape(-1)


def footprint(W, H, members):
    """members = (pw, ph, x, y, mask): regions of planes of level size (pw, ph), box (x, y) + mask.shape, boolean masks."""
    canvas = None
    boxes = []
    for pw, ph, x, y, mask in members:
        h, w = mask.shape
        xs, ys = samples(W, pw), samples(H, ph)
        c0, c1 = np.searchsorted(xs, x, "left"), np.searchsorted(xs, x + w, "left")
        r0, r1 = np.searchsorted(ys, y, "left"), np.searchsorted(ys, y + h, "left")
        if c0 >= c1 or r0 >= r1:
            continue
        boxes.append((int(c0), int(r0), int(c1), int(r1), mask[np.ix_(ys[r0:r1] - y, xs[c0:c1] - x)]))
    if not boxes:
        return Foot()
    x0, y0 = min(b[0] for b in boxes), min(b[1] for b in boxes)
    x1, y1 = max(b[2] for b in boxes), max(b[3] for b in boxes)
    canvas = np.zeros((y1 - y0, x1 - x0), bool)
    for c0, r0, c1, r1, sub in boxes:
        canvas[r0 - y0:r1 - y0, c0 - x0:c1 - x0] |= sub
    if not canvas.any():
        return Foot()
    rows, cols = np.nonzero(canvas.any(axis=1))[0], np.nonzero(canvas.any(axis=0))[0]
    return Foot(x0 + cols[0], y0 + rows[0], canvas[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1].copy())


def brute_footprint(W, H, members):
    """The pixel rule pixel by pixel: the (H, W) boolean footprint."""
    out = np.zeros((H, W), bool)
    for yy in range(H):
        for xx in range(W):
            for pw, ph, x, y, mask in members:
                xs, ys = ((2 * xx + 1) * pw) // (2 * W), ((2 * yy + 1) * ph) // (2 * H)
                h, w = mask.shape
                if x <= xs < x + w and y <= ys < y + h and mask[ys - y, xs - x]:
                    out[yy, xx] = True
    return out


def inter(a, b):
    """|F(a) & F(b)| by boolean AND over the frame (over the intersection of the two foot boxes: elsewhere one of them is empty)."""
    x0, y0 = max(a.x, b.x), max(a.y, b.y)
    x1, y1 = min(a.x + a.w, b.x + b.w), min(a.y + a.h, b.y + b.h)
    if x0 >= x1 or y0 >= y1:
        return 0
    return int((a.bits[y0 - a.y:y1 - a.y, x0 - a.x:x1 - a.x] & b.bits[y0 - b.y:y1 - b.y, x0 - b.x:x1 - b.x]).sum())


def all_pairs(feet, frames):
    """(a, b, inter) of every pair a < b of one frame with inter > 0, sorted by (a, b)."""
    out = []
    for a in range(len(feet)):
        for b in range(a + 1, len(feet)):
            if frames[a] == frames[b]:
                k = inter(feet[a], feet[b])
                if k > 0:
                    out.append((a, b, k))
    return out


def is_dup(pa, pb, k, num, den):
    return k > 0 and k * den >= num * (pa + pb - k)


def frame_lines(boxes, pixels, frames, pyr, pairs, num=1, den=2):
    """boxes[t] = (x, y, w, h), pixels[t], frames[t], pyr[t]; pairs = (a, b, inter).  Returns (dup per pair, frame_line per line,
    frame lines as dicts, members): components of the duplicate relation by a plain union-find, representative / order / levels by
    the contract."""
    n = len(pixels)
    parent = list(range(n))

    def find(t):
        while parent[t] != t:
            t = parent[t]
        return t

    dup = []
    for a, b, k in pairs:
        d = is_dup(int(pixels[a]), int(pixels[b]), int(k), num, den)
        dup.append(1 if d else 0)
        if d:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[rb] = ra
    comp = {}
    for t in range(n):
        comp.setdefault(find(t), []).append(t)
    groups = sorted(comp.values(), key=lambda g: (int(frames[g[0]]), min(g)))
    frame_line = [0] * n
    lines, members = [], []
    for i, g in enumerate(groups):
        g = sorted(g)
        rep = max(g, key=lambda t: (int(pixels[t]), -t))
        full = [t for t in g if boxes[t][2] > 0 and boxes[t][3] > 0]
        if full:
            x0, y0 = min(boxes[t][0] for t in full), min(boxes[t][1] for t in full)
            x1, y1 = max(boxes[t][0] + boxes[t][2] for t in full), max(boxes[t][1] + boxes[t][3] for t in full)
        else:
            x0 = y0 = x1 = y1 = 0
        levels = 0
        for t in g:
            frame_line[t] = i
            if pyr[t] < 32:
                levels |= 1 << int(pyr[t])
        lines.append(dict(frame=int(frames[g[0]]), rep=rep, first=len(members), count=len(g), x=int(x0), y=int(y0), w=int(x1 - x0), h=int(y1 - y0),
                          pixels=int(pixels[rep]), levels=levels))
        members += g
    return dup, frame_line, lines, members
