#!/usr/bin/env python3
"""Developer aid: what STR_ER_WANT_SHAPES costs.  The workloads of tools/dev_masks.py (pyr3x8: 32 S-text frames of 1920x1080,
{Y,Cr,Cb} x 8 levels; S-noise at the same size and config; the committed ICDAR crops), each on one context.  Four kinds of call
alternate -- plain, masks, shapes, masks + shapes -- in a rotating order; the call times are medians over --reps calls each.

    python tools/dev_shapes.py [--reps 11] [--out profiles/shapes.json]
    python tools/dev_shapes.py --iters 5 --only pyr3x8 --kind shapes    # flagged calls only, no timing (for rocprofv3 --kernel-trace --stats)
"""
import argparse, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: F401  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S
from dev_masks import workloads

KINDS = {"plain": (False, False), "masks": (True, False), "shapes": (False, True), "both": (True, True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--only", default="")
    ap.add_argument("--kind", default="shapes", choices=list(KINDS))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(); sp, wp = S.cascade_io.write_golden(tmp)
    out = {}
    for name, (prm, frames, is_list) in workloads().items():
        if a.only and name != a.only:
            continue
        f = S.ERFilter(params=S.Params(**prm))
        f.load_cascade(0, sp); f.load_cascade(1, wp)

        def call(kind):
            m, s = KINDS[kind]
            if is_list:
                return f.text_detect_list(frames, want_masks=m, want_shapes=s)
            return f.text_detect(frames, want_masks=m, want_shapes=s)

        res = {k: call(k) for k in KINDS}            # (warm-up: the buffers are made by the first flagged calls)
        assert all(r.cands.tobytes() == res["plain"].cands.tobytes() for r in res.values())
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
            for k in order[r % 4:] + order[:r % 4]:
                t0 = time.perf_counter()
                call(k)
                t[k].append((time.perf_counter() - t0) * 1e3)
        sh = res["shapes"].shapes
        med = {k: float(np.median(v)) for k, v in t.items()}
        out[name] = {"frames": len(frames), "cands": len(sh), "holes": int((sh["hole_pixels"] > 0).sum()),
                     **{f"ms_{k}_median": med[k] for k in KINDS},
                     "shapes_vs_plain": med["shapes"] / med["plain"] - 1.0, "shapes_vs_masks": med["shapes"] / med["masks"] - 1.0,
                     **{f"ms_{k}_all": t[k] for k in KINDS}}
        print(json.dumps({name: {k: v for k, v in out[name].items() if not k.endswith("_all")}}), flush=True)
        f.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
