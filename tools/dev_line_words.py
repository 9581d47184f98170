#!/usr/bin/env python3
"""Developer aid: what STR_ER_WANT_LINE_WORDS costs on the pyr3x8 workload of tools/dev_frame_lines.py (48 S-text frames of 1920x1080,
{Y,Cr,Cb} x 8 levels), grouped stages.  Two kinds of call alternate -- grouped + frame lines, and the same with the line words -- and
every call time is printed (--reps calls each) with its median, minimum and maximum.  Also printed: the counts (lines, runs, words,
the most runs and words of a line) and the bytes of the three tables.  With STR_ER_DEBUG_STATS=1 the library prints the run slots it
reserved, the bytes copied back and the host time of the step.  --root runs another checkout of the library (one without the flag
measures the frame-line call alone: the flag-off cost of a change is the difference of two such runs).

    python tools/dev_line_words.py [--reps 5] [--frames 48] [--root DIR] [--out profiles/line_words.json]
    python tools/dev_line_words.py --iters 5       # flagged calls only, no timing (for rocprofv3 --kernel-trace --stats)
"""
import argparse, json, os, sys, tempfile, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--iters", type=int, default=0)
ap.add_argument("--frames", type=int, default=48)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import torch  # noqa: F401,E402  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S  # noqa: E402

GROUPED = S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP
KINDS = {"frame_lines": GROUPED | S.WANT_FRAME_LINES}
if hasattr(S, "WANT_LINE_WORDS"):
    KINDS["frame_lines_words"] = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS
    # the geometry beside it: k_foot_geom in the same kernel trace
    KINDS["frame_lines_words_geom"] = GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS | S.WANT_LINE_GEOM


def main():
    tmp = tempfile.mkdtemp(); sp, wp = S.cascade_io.write_golden(tmp)
    sy = S.synth
    frames = np.stack([sy.stext_bgr(sy.frame_seed(i), 1920, 1080) for i in range(a.frames)])
    f = S.ERFilter(params=S.Params(max_width=1920, max_height=1080, max_frames=a.frames, n_pyr_levels=8, channel_mask=0x07))
    f.load_cascade(0, sp); f.load_cascade(1, wp)
    res = {k: f.text_detect(frames, st) for k, st in KINDS.items()}           # (warm-up: the buffers are made by the first flagged calls)
    for _ in range(2):
        for st in KINDS.values():
            f.text_detect(frames, st)
    r = res["frame_lines"]
    out = {"root": os.path.abspath(a.root), "frames": a.frames, "lines": len(r.texts), "frame_lines": len(r.frame_lines)}
    if "frame_lines_words" in res:
        g = res["frame_lines_words"]
        assert g.line_feet.tobytes() == r.line_feet.tobytes() and g.frame_lines.tobytes() == r.frame_lines.tobytes()
        out.update(runs=len(g.line_runs), words=len(g.words), most_runs=int(g.line_words["n_runs"].max(initial=0)),
                   most_words=int(g.line_words["n_words"].max(initial=0)), largest_colmax=int(g.line_words["colmax"].max(initial=0)),
                   table_bytes=int(g.line_words.nbytes + g.line_runs.nbytes + g.words.nbytes))
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
        if "frame_lines_words" in t:
            out["added_ms"] = round(out["frame_lines_words_ms"]["median"] - out["frame_lines_ms"]["median"], 3)
    f.close()
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
