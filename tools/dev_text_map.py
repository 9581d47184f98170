#!/usr/bin/env python3
"""Developer aid: what STR_ER_WANT_TEXT_MAP / _LINE_MAP cost.  pyr3x8 (48 S-text frames of 1920x1080, {Y,Cr,Cb} x 8 levels) and the
committed ICDAR crops (a list of 4 frames, 6 planes), each on one context.  Six kinds of call alternate in a rotating order -- plain,
text map, masks, masks + text map, grouped, grouped + both maps -- and the call times are medians over --reps calls each.

    python tools/dev_text_map.py [--reps 9] [--out profiles/text_map.json]
    python tools/dev_text_map.py --iters 5 --only pyr3x8 --kind map     # flagged calls only, no timing (for rocprofv3 --kernel-trace --stats)
    STR_ER_DEBUG_STATS=1 python tools/dev_text_map.py --iters 2 --only pyr3x8 --kind masks_map 2>&1 | grep "text map:"   # host binning
"""
import argparse, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S

GROUPED = S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP
KINDS = {"plain": S.STAGE_ALL, "map": S.STAGE_ALL | S.WANT_TEXT_MAP, "masks": S.STAGE_ALL | S.WANT_MASKS,
         "masks_map": S.STAGE_ALL | S.WANT_MASKS | S.WANT_TEXT_MAP, "group": GROUPED, "group_maps": GROUPED | S.WANT_TEXT_MAP | S.WANT_LINE_MAP}


def workloads():
    sy = S.synth
    z = np.load(os.path.join(ROOT, "tests", "golden", "icdar_crops.npz"))
    return {
        "pyr3x8": (dict(max_width=1920, max_height=1080, max_frames=48, n_pyr_levels=8, channel_mask=0x07),
                   np.stack([sy.stext_bgr(sy.frame_seed(i), 1920, 1080) for i in range(48)]), False),
        "icdar": (dict(max_width=640, max_height=480, max_frames=8), [np.ascontiguousarray(z[k]) for k in sorted(z.files)], True),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--only", default="")
    ap.add_argument("--kind", default="map", choices=list(KINDS))
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
            return f.text_detect_list(frames, KINDS[kind]) if is_list else f.text_detect(frames, KINDS[kind])

        res = {k: call(k) for k in KINDS}            # (warm-up: the buffers are made by the first flagged calls)
        assert all(r.cands.tobytes() == res["plain"].cands.tobytes() for r in res.values())
        assert res["map"].text_map_pixels.tobytes() == res["masks_map"].text_map_pixels.tobytes()
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
        med = {k: float(np.median(v)) for k, v in t.items()}
        c = res["plain"].cands
        tm = res["group_maps"].text_map_pixels
        out[name] = {"frames": len(frames), "cands": len(c), "strong_weak": int((c["cls"] != 0).sum()), "lines": len(res["group"].texts),
                     "text_pixels": int(((res["map"].text_map_pixels & 3) != 0).sum()), "map_elements": int(len(res["map"].text_map_pixels)),
                     "d2h_bytes_map": int(len(res["map"].text_map_pixels)), "d2h_bytes_both": int(len(tm) * 5),
                     **{f"ms_{k}_median": med[k] for k in KINDS},
                     "map_vs_plain": med["map"] / med["plain"] - 1.0, "map_vs_masks": med["masks_map"] / med["masks"] - 1.0,
                     "maps_vs_group": med["group_maps"] / med["group"] - 1.0,
                     **{f"ms_{k}_all": t[k] for k in KINDS}}
        print(json.dumps({name: {k: v for k, v in out[name].items() if not k.endswith("_all")}}), flush=True)
        f.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
