#!/usr/bin/env python3
"""Developer aid: what STR_ER_WANT_LINE_CROPS / _GLYPHS cost.  The bench's pyr3x8 batch (32 S-text frames of 1920x1080, {Y,Cr,Cb} x 8
levels) with STAGE_ALL | TRACK | GROUP | GROUP_INNER_SUP on one context, three versions: without the flags, + WANT_LINE_CROPS and
+ WANT_LINE_GLYPHS.  The versions alternate; each takes --regions regions of at least --region-s seconds of back-to-back calls, and a
region's time per call is its wall time over its calls; the report is the median region.  Also reports the lines, members and crop
bytes per call.

    python tools/dev_line_crops.py [--regions 7] [--region-s 0.5] [--out profiles/line_crops.json]
    python tools/dev_line_crops.py --iters 5 --glyphs     # flagged calls only, no timing (for a rocprofv3 --kernel-trace --stats run)
"""
import argparse, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S

STAGES = S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP | S.GROUP_INNER_SUP
VERSIONS = {"plain": 0, "crops": S.WANT_LINE_CROPS, "glyphs": S.WANT_LINE_CROPS | S.WANT_LINE_GLYPHS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--region-s", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--glyphs", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(); sp, wp = S.cascade_io.write_golden(tmp)
    sy = S.synth
    frames = np.stack([sy.stext_bgr(sy.frame_seed(i), 1920, 1080) for i in range(32)])
    f = S.ERFilter(params=S.Params(max_width=1920, max_height=1080, max_frames=32, n_pyr_levels=8, channel_mask=0x07))
    f.load_cascade(0, sp); f.load_cascade(1, wp)
    call = lambda flags: f.text_detect(frames, STAGES | flags)          # noqa: E731
    res = {k: call(v) for k, v in VERSIONS.items()}                     # (warm-up: the crop and mask buffers are made by the first flagged call)
    assert res["plain"].texts.tobytes() == res["crops"].texts.tobytes() == res["glyphs"].texts.tobytes()
    assert res["crops"].line_crop_pixels.tobytes() == res["glyphs"].line_crop_pixels.tobytes()
    if a.iters:
        for _ in range(a.iters):
            call(VERSIONS["glyphs" if a.glyphs else "crops"])
        print(json.dumps({"iters": a.iters, "lines": len(res["crops"].texts)}))
        f.close()
        return
    per_call = {k: [] for k in VERSIONS}
    names = list(VERSIONS)
    for r in range(a.regions):
        for k in (names if r % 2 == 0 else names[::-1]):
            n, t0 = 0, time.perf_counter()
            while True:
                call(VERSIONS[k])
                n += 1
                el = time.perf_counter() - t0
                if el >= a.region_s:
                    break
            per_call[k].append(el / n * 1e3)
    g = res["glyphs"]
    med = {k: float(np.median(v)) for k, v in per_call.items()}
    out = {"frames": len(frames), "stages": STAGES, "lines": int(len(g.texts)), "members": int(len(g.text_ers)),
           "distinct_members": int(len(np.unique(g.text_ers))), "crop_bytes": int(len(g.line_crop_pixels)),
           "crop_pixels": int((g.line_crops["width"].astype(np.int64) * g.line_crops["height"]).sum()),
           "widest": int(g.line_crops["width"].max()) if len(g.texts) else 0,
           "ms_plain_median": med["plain"], "ms_crops_median": med["crops"], "ms_glyphs_median": med["glyphs"],
           "overhead_crops": med["crops"] / med["plain"] - 1.0, "overhead_glyphs": med["glyphs"] / med["plain"] - 1.0,
           "ms_per_region": per_call}
    print(json.dumps({k: v for k, v in out.items() if k != "ms_per_region"}), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    f.close()


if __name__ == "__main__":
    main()
