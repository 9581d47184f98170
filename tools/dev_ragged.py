#!/usr/bin/env python3
"""Developer aid: 32 frames of four sizes (8 each of 1920x1080, 1280x720, 1024x768, 641x359, S-text, shuffled) three ways in one process:
(a) one str_er_detect_bgr_list call, (b) grouped by size into four uniform str_er_detect_bgr calls, (c) one call per frame.  Rounds alternate
the order of the three; each timed region runs >= --min-s seconds; frames/s = median over --rounds rounds.

    python tools/dev_ragged.py --config pyr3x8|native6 [--out profiles/ragged_<config>.json]
    python tools/dev_ragged.py --config pyr3x8 --iters 5      # fixed number of calls per way, no timing (for a rocprofv3 --kernel-trace run)
"""
import argparse, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S

SIZES = [(1920, 1080), (1280, 720), (1024, 768), (641, 359)]
CONFIGS = {"pyr3x8": dict(n_pyr_levels=8, channel_mask=0x07), "native6": dict(n_pyr_levels=1, channel_mask=0x3F)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="pyr3x8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(); sp, wp = S.cascade_io.write_golden(tmp)
    f = S.ERFilter(params=S.Params(max_width=1920, max_height=1080, max_frames=32, **CONFIGS[a.config]))
    f.load_cascade(0, sp); f.load_cascade(1, wp)
    frames = [S.synth.stext_bgr(S.synth.frame_seed(100 * k + i), w, h) for k, (w, h) in enumerate(SIZES) for i in range(8)]
    order = np.random.default_rng(7).permutation(len(frames))
    frames = [frames[i] for i in order]
    groups = {s: np.stack([fr for fr in frames if (fr.shape[1], fr.shape[0]) == s]) for s in SIZES}

    def way_a():
        return len(f.text_detect_list(frames).cands)

    def way_b():
        return sum(len(f.text_detect(g).cands) for g in groups.values())

    def way_c():
        return sum(len(f.text_detect(fr).cands) for fr in frames)

    ways = {"a_list": way_a, "b_grouped": way_b, "c_per_frame": way_c}
    n_a, n_b, n_c = way_a(), way_b(), way_c()        # (warm-up; and the three ways find the same candidates)
    assert n_a == n_b == n_c, (n_a, n_b, n_c)
    if a.iters:
        for name, fn in ways.items():
            for _ in range(a.iters):
                fn()
        print(json.dumps({"config": a.config, "iters": a.iters, "cands": n_a}))
        return
    fps = {k: [] for k in ways}
    names = list(ways)
    for r in range(a.rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            fn, n, t0 = ways[name], 0, time.perf_counter()
            while True:
                fn(); n += 1
                dt = time.perf_counter() - t0
                if dt >= a.min_s:
                    break
            fps[name].append(n * len(frames) / dt)
    med = {k: float(np.median(v)) for k, v in fps.items()}
    out = {"config": a.config, "frames": len(frames), "sizes": SIZES, "rounds": a.rounds, "min_s": a.min_s, "cands": n_a,
           "frames_per_s_median": med, "frames_per_s_all": fps,
           "a_over_c": med["a_list"] / med["c_per_frame"], "a_over_b": med["a_list"] / med["b_grouped"]}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
