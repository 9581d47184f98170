#!/usr/bin/env python3
"""Developer aid: what STR_ER_WANT_MASKS costs.  Three workloads, each on one context: the bench's pyr3x8 (32 S-text frames of
1920x1080, {Y,Cr,Cb} x 8 levels), S-noise at the same size and config, and the committed ICDAR crops (one list call, six planes).
Calls with and without the flag alternate; the call times are medians over --reps calls each.  Also reports the candidates, the
mask words and pixels per call, and how many boxes each kernel size class takes.

    python tools/dev_masks.py [--reps 15] [--out profiles/masks.json]
    python tools/dev_masks.py --iters 5 --only pyr3x8      # masked calls only, no timing (for a rocprofv3 --kernel-trace --stats run)
"""
import argparse, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S


def workloads():
    sy = S.synth
    z = np.load(os.path.join(ROOT, "tests", "golden", "icdar_crops.npz"))
    pyr = dict(max_width=1920, max_height=1080, max_frames=32, n_pyr_levels=8, channel_mask=0x07)
    return {
        "pyr3x8": (pyr, np.stack([sy.stext_bgr(sy.frame_seed(i), 1920, 1080) for i in range(32)]), False),
        "snoise": (pyr, np.stack([sy.snoise_bgr(sy.frame_seed(100 + i), 1920, 1080) for i in range(32)]), False),
        "icdar": (dict(max_width=640, max_height=480, max_frames=8), [np.ascontiguousarray(z[k]) for k in sorted(z.files)], True),
    }


def size_class(w, h):          # er_masks.inl: mask_class
    if w <= 64 and h <= 64:
        return 0
    return 1 if h * ((w + 63) // 64) <= 1024 else 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(); sp, wp = S.cascade_io.write_golden(tmp)
    out = {}
    for name, (prm, frames, is_list) in workloads().items():
        if a.only and name != a.only:
            continue
        f = S.ERFilter(params=S.Params(**prm))
        f.load_cascade(0, sp); f.load_cascade(1, wp)

        def call(masks):
            if is_list:
                return f.text_detect_list(frames, want_masks=masks)
            return f.text_detect(frames, want_masks=masks)

        plain, masked = call(False), call(True)          # (warm-up: the mask buffers are made by the first flagged call)
        assert plain.cands.tobytes() == masked.cands.tobytes()
        if a.iters:
            for _ in range(a.iters):
                call(True)
            out[name] = {"iters": a.iters, "cands": len(masked.cands)}
            f.close()
            continue
        t = {False: [], True: []}
        for r in range(a.reps):
            for m in ((False, True) if r % 2 == 0 else (True, False)):
                t0 = time.perf_counter()
                call(m)
                t[m].append(time.perf_counter() - t0)
        c = masked.cands
        cls = np.array([size_class(int(w), int(h)) for w, h in zip(c["w"], c["h"])], np.int64)
        med0, med1 = float(np.median(t[False])) * 1e3, float(np.median(t[True])) * 1e3
        out[name] = {"frames": len(frames), "cands": len(c), "mask_words": int(len(masked.mask_bits)),
                     "mask_pixels": int(masked.mask_pixels.sum()), "box_pixels": int((c["w"].astype(np.int64) * c["h"]).sum()),
                     "boxes_per_class": [int((cls == k).sum()) for k in range(3)],
                     "largest_box": [int(c["w"].max()), int(c["h"].max())] if len(c) else [0, 0],
                     "ms_plain_median": med0, "ms_masks_median": med1, "overhead": med1 / med0 - 1.0,
                     "ms_plain_all": t[False], "ms_masks_all": t[True]}
        print(json.dumps({name: {k: v for k, v in out[name].items() if not k.endswith("_all")}}), flush=True)
        f.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
