#!/usr/bin/env python3
"""Developer aid: what STR_ER_WANT_RUN_READ costs on the pyr3x8 text workload ({Y,Cr,Cb} x 8 levels, 32 S-text frames of 1920x1080 in
one call), grouped stages.  Two kinds of call alternate -- grouped + frame lines + line words, and the same with the run reading --
and every call time is printed (--reps calls each) with its median, minimum and maximum.  Also printed: the counts (lines, runs,
words), the atlas (bytes, how often it grew), the bytes of the tiles themselves and a few strings.  With STR_ER_DEBUG_STATS=1 the
library prints the atlas of every flagged call.  --root runs another checkout of the library (one without the flag measures the
line-words call alone: the spread of the parent).

    python tools/dev_run_read.py [--reps 7] [--frames 32] [--root DIR] [--plain] [--out FILE]
    python tools/dev_run_read.py --iters 5       # flagged calls only, no timing (for rocprofv3 --kernel-trace --stats)
"""
import argparse, gzip, json, os, sys, tempfile, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=0)
ap.add_argument("--frames", type=int, default=32)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--plain", action="store_true", help="the line-words calls only, as a checkout without the flag runs them")
ap.add_argument("--out", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import torch  # noqa: F401,E402  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S  # noqa: E402

GROUPED = S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP
KINDS = {"line_words": GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS}
if hasattr(S, "WANT_RUN_READ") and not a.plain:
    KINDS["run_read"] = KINDS["line_words"] | S.WANT_RUN_READ


def main():
    tmp = tempfile.mkdtemp(); sp, wp = S.cascade_io.write_golden(tmp)
    model = os.path.join(tmp, "ocr.model")
    with open(model, "wb") as fh:
        fh.write(gzip.open(S.cascade_io.ocr_model_path(120)).read())
    sy = S.synth
    frames = np.stack([sy.stext_bgr(sy.frame_seed(i), 1920, 1080) for i in range(a.frames)])
    f = S.ERFilter(params=S.Params(max_width=1920, max_height=1080, max_frames=a.frames, n_pyr_levels=8, channel_mask=0x07))
    f.load_cascade(0, sp); f.load_cascade(1, wp)
    f.load_svm_model(model, 1800)
    res = {k: f.text_detect(frames, st) for k, st in KINDS.items()}           # (warm-up: the buffers are made by the first flagged calls)
    for _ in range(2):
        for st in KINDS.values():
            f.text_detect(frames, st)
    r = res["line_words"]
    out = {"root": os.path.abspath(a.root), "frames": a.frames, "lines": len(r.texts), "runs": len(r.line_runs), "words": len(r.words)}
    if "run_read" in res:
        g = res["run_read"]
        assert g.line_runs.tobytes() == r.line_runs.tobytes() and g.words.tobytes() == r.words.tobytes()
        w = (g.line_runs["x1"] - g.line_runs["x0"]).astype(np.int64); h = (g.line_runs["y1"] - g.line_runs["y0"]).astype(np.int64)
        atlas, grown = f.run_atlas_stats()
        out.update(atlas_bytes=atlas, atlas_grown=grown, tile_bytes=int((((w + 3) // 4 * 4) * h).sum()), widest_run=int(w.max(initial=0)),
                   tallest_run=int(h.max(initial=0)), median_prob=round(float(np.median(g.run_reads["prob"])), 4) if len(w) else None,
                   texts=[g.frame_line_text(i) for i in range(min(8, len(g.frame_lines)))])
    if a.iters:
        for _ in range(a.iters):
            f.text_detect(frames, list(KINDS.values())[-1])
        out["iters"] = a.iters
    else:
        t = {k: [] for k in KINDS}
        order = list(KINDS)
        for i in range(a.reps):
            for k in order[i % len(order):] + order[:i % len(order)]:
                t0 = time.perf_counter()
                f.text_detect(frames, KINDS[k])
                t[k].append(round((time.perf_counter() - t0) * 1e3, 3))
        for k in KINDS:
            out[k + "_ms"] = {"calls": t[k], "median": round(float(np.median(t[k])), 3), "min": min(t[k]), "max": max(t[k])}
        if "run_read" in t:
            out["added_ms"] = round(out["run_read_ms"]["median"] - out["line_words_ms"]["median"], 3)
    f.close()
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
