#!/usr/bin/env python3
"""Records per group of tiles of S-text frames at pyr3x8, by class of planes: what k_group_merge's tables have to hold.

    python tools/group_census.py [--frames 0-7] [--gx 8 --gy 4] [--width 1920 --height 1080] [--levels 8]

No GPU: the frames are the benchmark's (synth.stext_bgr), the planes the oracle's (compute_channels, pyramid), the records the census of
tests/tree_planes.py -- which the tests prove equal to last_tree_stats()["records"].  Luma planes are the small k_tile_tree's (fold limit 332),
chroma planes k_tile_tree2's with the tiles it hands back.  Seconds per frame.  profiles/group_bins.md holds the table of frames 0-7.
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tree_planes as tp  # noqa: E402

TABLES = (512, 1024, 2048, 2528)


def group_records(c, gx, gy, tile2):
    """Records of every group of gx x gy tiles of a census (tile2: the plane is k_tile_tree2's)."""
    if not tile2:
        return c.group_records(gx, gy, tp.SPARSE_FOLD).ravel()
    try:
        back = c.tile2_outcome()[1]
    except AssertionError:          # (a pair past two of k_tile_tree2's limits at once: the census does not say which tiles come back -- count them all as handed back)
        back = set(c.tiles)
    e = np.array([[c.tiles[y, x].exported(tp.SPARSE_FOLD) if (y, x) in back else c.tiles[y, x].fold_exported for x in range(c.tiles_x)]
                  for y in range(c.tiles_y)])
    return np.array([int(e[y:y + gy, x:x + gx].sum()) for y in range(0, c.tiles_y, gy) for x in range(0, c.tiles_x, gx)])


def frame_groups(o, S, index, w, h, levels, gx, gy):
    """class of planes -> records of its groups with at least two tiles, one frame."""
    six = o.compute_channels(S.synth.stext_bgr(S.synth.frame_seed(index), w, h))
    out = {"chroma": [], "luma level 0": [], "luma levels 1-%d" % (levels - 1): []}
    for ch in range(3):
        for lv, p in enumerate(o.pyramid(six[ch], levels)):
            c = tp.Census(p, 8, 120)
            g = group_records(c, gx, gy, tile2=ch != 0)
            ntiles = np.array([min(gx, c.tiles_x - x) * min(gy, c.tiles_y - y) for y in range(0, c.tiles_y, gy) for x in range(0, c.tiles_x, gx)])
            key = "chroma" if ch else ("luma level 0" if lv == 0 else "luma levels 1-%d" % (levels - 1))
            out[key].extend(int(v) for v in g[ntiles >= 2])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", default="0-7", help="first-last or one index")
    ap.add_argument("--gx", type=int, default=8)
    ap.add_argument("--gy", type=int, default=4)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--levels", type=int, default=8)
    a = ap.parse_args()
    lo, _, hi = a.frames.partition("-")
    frames = range(int(lo), int(hi or lo) + 1)
    from oracle.oracle import Oracle
    S = importlib.import_module("scene-text-recognition_amd")
    o = Oracle()
    total = {}
    for i in frames:
        for k, v in frame_groups(o, S, i, a.width, a.height, a.levels, a.gx, a.gy).items():
            total.setdefault(k, []).extend(v)
            big = [x for x in v if x > TABLES[2]]
            if big:
                print("frame %d, %s: groups above %d records: %s" % (i, k, TABLES[2], sorted(big)), file=sys.stderr)
    n = len(frames)
    print("| class of planes | groups / frame | p50 | p90 | p99 | max | " + " | ".join("> %d" % t for t in TABLES) + " | share of records |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    all_records = sum(sum(v) for v in total.values())
    for k, v in total.items():
        v = np.array(v)
        print("| %s | %.0f | %d | %d | %d | %d | %s | %.2f |" % (k, len(v) / n, *(int(np.percentile(v, q)) for q in (50, 90, 99)), int(v.max()),
                                                                 " | ".join("%.1f" % ((v > t).sum() / n) for t in TABLES), v.sum() / all_records))
    print("records per frame: %.0f" % (all_records / n))


if __name__ == "__main__":
    main()
