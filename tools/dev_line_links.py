#!/usr/bin/env python3
"""Developer aid: what STR_ER_WANT_LINE_LINKS costs on a moving-window video on the pyr3x8 context of tools/dev_frame_lines.py (48
frames of 1920x1080 cut out of one larger S-text canvas, the window moving --motion pixels a frame; {Y,Cr,Cb} x 8 levels), grouped
stages.  Two kinds of call alternate in a rotating order -- grouped + frame lines, grouped + frame lines + line links -- and the call
times are medians over --reps calls each.  Also printed: the counts (lines, overlaps across adjacent frames, links, tracks, the longest
track) and the bytes of the tables and of the edge feet.  With STR_ER_DEBUG_STATS=1 the library prints the candidate pairs and the
bytes copied back for the link table and for the edge feet.

    python tools/dev_line_links.py [--reps 9] [--frames 48] [--motion 3 1] [--out profiles/line_links.json]
    python tools/dev_line_links.py --iters 5       # flagged calls only, no timing (for rocprofv3 --kernel-trace --stats)
"""
import argparse, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S

GROUPED = S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP
KINDS = {"frame_lines": GROUPED | S.WANT_FRAME_LINES, "frame_lines_links": GROUPED | S.WANT_FRAME_LINES | S.WANT_LINE_LINKS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--motion", type=int, nargs=2, default=(3, 1))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(); sp, wp = S.cascade_io.write_golden(tmp)
    sy = S.synth
    mx, my = a.motion
    canvas = sy.stext_bgr(sy.frame_seed(0), 1920 + mx * a.frames, 1080 + my * a.frames)
    frames = np.stack([canvas[my * i:my * i + 1080, mx * i:mx * i + 1920] for i in range(a.frames)])
    f = S.ERFilter(params=S.Params(max_width=1920, max_height=1080, max_frames=a.frames, n_pyr_levels=8, channel_mask=0x07))
    f.load_cascade(0, sp); f.load_cascade(1, wp)
    res = {k: f.text_detect(frames, st) for k, st in KINDS.items()}           # (warm-up: the buffers are made by the first flagged calls)
    r, p = res["frame_lines_links"], res["frame_lines"]
    assert all(getattr(r, k).tobytes() == getattr(p, k).tobytes() for k in ("cands", "texts", "line_feet", "line_pairs", "frame_lines", "frame_line_members"))
    tr = r.text_tracks
    edge = [r.edge_feet(0), r.edge_feet(1)]
    out = {"frames": a.frames, "motion": [mx, my], "lines": len(r.texts), "pairs": len(r.line_pairs), "overlaps": len(r.line_links),
           "links": int(r.line_links["link"].sum()), "tracks": len(tr), "longest_track_frames": int((tr["last_frame"] - tr["first_frame"]).max() + 1) if len(tr) else 0,
           "tracks_over_all_frames": int(((tr["first_frame"] == 0) & (tr["last_frame"] == a.frames - 1)).sum()),
           "table_bytes": int(r.line_links.nbytes + r.line_tracks.nbytes + tr.nbytes + r.text_track_members.nbytes),
           "edge_feet_lines": [len(e.lines) for e in edge], "edge_feet_result_bytes": [int(e.bits.nbytes + e.feet.nbytes + e.lines.nbytes) for e in edge]}
    if a.iters:
        for _ in range(a.iters):
            f.text_detect(frames, KINDS["frame_lines_links"])
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
        out["added_ms"] = round(out["frame_lines_links_ms"]["median"] - out["frame_lines_ms"]["median"], 3)
    f.close()
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
