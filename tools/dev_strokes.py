#!/usr/bin/env python3
"""Developer aid: what STR_ER_WANT_STROKES costs.  The workloads of tools/dev_masks.py (pyr3x8: 32 S-text frames of 1920x1080,
{Y,Cr,Cb} x 8 levels; S-noise at the same size and config; the committed ICDAR crops), each on one context.  Five kinds of call
alternate -- plain, masks, shapes, strokes, shapes + strokes -- in a rotating order; the call times are medians over --reps calls each.
Also reported: the distribution of K (depth_max) over the candidates, and the rows the stroke sweep visits per size class, counted
on the CPU from the masks with the reference (tests/stroke_ref.py) for the first --rows-frames frames of a workload.

    python tools/dev_strokes.py [--reps 11] [--out profiles/strokes.json]
    python tools/dev_strokes.py --iters 5 --only pyr3x8 --kind strokes   # flagged calls only, no timing (for rocprofv3 --kernel-trace --stats)
"""
import argparse, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S
from dev_masks import size_class, workloads
from stroke_ref import depth

KINDS = {"plain": (False, False, False), "masks": (True, False, False), "shapes": (False, True, False), "strokes": (False, False, True),
         "both": (False, True, True)}


def rows_swept(mask):
    """The rows the kernels' sweep visits for one mask: step 1 the whole box, step k + 1 the rows from the first to the last that
    hold a pixel of E_{k-1} = {D >= k}."""
    d = depth(mask)
    rows = d.max(axis=1)
    n = mask.shape[0]
    for k in range(1, int(d.max())):
        ys = np.nonzero(rows >= k)[0]
        n += int(ys[-1] - ys[0] + 1)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--only", default="")
    ap.add_argument("--kind", default="strokes", choices=list(KINDS))
    ap.add_argument("--rows-frames", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(); sp, wp = S.cascade_io.write_golden(tmp)
    out = {}
    for name, (prm, frames, is_list) in workloads().items():
        if a.only and name != a.only:
            continue
        f = S.ERFilter(params=S.Params(**prm))
        f.load_cascade(0, sp); f.load_cascade(1, wp)

        def call(kind, fr=frames):
            m, s, k = KINDS[kind]
            if is_list:
                return f.text_detect_list(fr, want_masks=m, want_shapes=s, want_strokes=k)
            return f.text_detect(fr, want_masks=m, want_shapes=s, want_strokes=k)

        res = {k: call(k) for k in KINDS}            # (warm-up: the buffers are made by the first flagged calls)
        assert all(r.cands.tobytes() == res["plain"].cands.tobytes() for r in res.values())
        assert res["strokes"].strokes.tobytes() == res["both"].strokes.tobytes()
        assert res["shapes"].shapes.tobytes() == res["both"].shapes.tobytes()
        if a.iters:
            for _ in range(a.iters):
                call(a.kind)
            out[name] = {"iters": a.iters, "kind": a.kind, "cands": len(res["plain"].cands)}
            f.close()
            continue
        t = {k: [] for k in KINDS}
        order = list(KINDS)
        for r in range(a.reps):
            for k in order[r % len(order):] + order[:r % len(order)]:
                t0 = time.perf_counter()
                call(k)
                t[k].append((time.perf_counter() - t0) * 1e3)
        st = res["strokes"].strokes
        kk = st["depth_max"].astype(np.int64)
        hist = {int(v): int(c) for v, c in zip(*np.unique(kk, return_counts=True))}
        # rows swept per size class, on the first frames (the reference counts them from the masks)
        sub = frames[:a.rows_frames]
        mres = call("masks", sub)
        swept = {0: [0, 0, 0], 1: [0, 0, 0], 2: [0, 0, 0]}             # boxes, box rows, rows swept
        for i, c in enumerate(mres.cands):
            sc = size_class(int(c["w"]), int(c["h"]))
            swept[sc][0] += 1
            swept[sc][1] += int(c["h"])
            swept[sc][2] += rows_swept(mres.mask(i))
        med = {k: float(np.median(v)) for k, v in t.items()}
        out[name] = {"frames": len(frames), "cands": len(st), "K_hist": hist, "K_mean": float(kk.mean()), "K_max": int(kk.max()),
                     "rows_swept_frames": len(sub),
                     "rows_swept_by_class": {str(c): {"boxes": v[0], "box_rows": v[1], "rows_swept": v[2]} for c, v in swept.items()},
                     **{f"ms_{k}_median": med[k] for k in KINDS},
                     "strokes_vs_plain": med["strokes"] / med["plain"] - 1.0, "strokes_vs_masks": med["strokes"] / med["masks"] - 1.0,
                     "both_vs_shapes": med["both"] / med["shapes"] - 1.0,
                     **{f"ms_{k}_all": t[k] for k in KINDS}}
        print(json.dumps({name: {k: v for k, v in out[name].items() if not k.endswith("_all") and k != "K_hist"}}), flush=True)
        f.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
