#!/usr/bin/env python3
"""Developer aid: what STR_ER_WANT_FRAME_LINES costs on the pyr3x8 workload of tools/dev_text_map.py (48 S-text frames of 1920x1080,
{Y,Cr,Cb} x 8 levels), grouped stages.  Three kinds of call alternate in a rotating order -- grouped, grouped + frame lines,
grouped + the byte map (the dense alternative) -- and the call times are medians over --reps calls each.  Also printed: the counts
(lines, pairs with common pixels, duplicates, frame lines, frame lines with members of two or more levels) and the bytes of the four
tables.  With STR_ER_DEBUG_STATS=1 the library prints the candidate pairs, the bytes copied back and the host time of the phase.

    python tools/dev_frame_lines.py [--reps 9] [--frames 48] [--out profiles/frame_lines.json]
    python tools/dev_frame_lines.py --iters 5       # flagged calls only, no timing (for rocprofv3 --kernel-trace --stats)
"""
import argparse, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S

GROUPED = S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP
KINDS = {"group": GROUPED, "group_frame_lines": GROUPED | S.WANT_FRAME_LINES, "group_text_map": GROUPED | S.WANT_TEXT_MAP}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(); sp, wp = S.cascade_io.write_golden(tmp)
    sy = S.synth
    frames = np.stack([sy.stext_bgr(sy.frame_seed(i), 1920, 1080) for i in range(a.frames)])
    f = S.ERFilter(params=S.Params(max_width=1920, max_height=1080, max_frames=a.frames, n_pyr_levels=8, channel_mask=0x07))
    f.load_cascade(0, sp); f.load_cascade(1, wp)
    res = {k: f.text_detect(frames, st) for k, st in KINDS.items()}           # (warm-up: the buffers are made by the first flagged calls)
    assert all(r.cands.tobytes() == res["group"].cands.tobytes() and r.texts.tobytes() == res["group"].texts.tobytes() for r in res.values())
    r = res["group_frame_lines"]
    fl = r.frame_lines
    multi = int(sum(bin(int(v)).count("1") >= 2 for v in fl["levels"]))
    out = {"frames": a.frames, "cands": len(r.cands), "lines": len(r.texts), "pairs": len(r.line_pairs), "duplicates": int(r.line_pairs["dup"].sum()),
           "frame_lines": len(fl), "frame_lines_multi_level": multi, "share_multi_level": round(multi / max(1, len(fl)), 4),
           "table_bytes": int(r.line_feet.nbytes + r.line_pairs.nbytes + fl.nbytes + r.frame_line_members.nbytes)}
    if a.iters:
        for _ in range(a.iters):
            f.text_detect(frames, KINDS["group_frame_lines"])
        out["iters"] = a.iters
    else:
        t = {k: [] for k in KINDS}
        order = list(KINDS)
        for i in range(a.reps):
            for k in order[i % len(order):] + order[:i % len(order)]:
                t0 = time.perf_counter()
                f.text_detect(frames, KINDS[k])
                t[k].append((time.perf_counter() - t0) * 1e3)
        for k in KINDS:
            out[k + "_ms"] = {"median": round(float(np.median(t[k])), 3), "min": round(min(t[k]), 3), "max": round(max(t[k]), 3)}
        out["added_ms"] = {k: round(out[k + "_ms"]["median"] - out["group_ms"]["median"], 3) for k in ("group_frame_lines", "group_text_map")}
    f.close()
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
