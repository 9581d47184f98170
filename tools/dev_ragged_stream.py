#!/usr/bin/env python3
"""Developer aid: the 32-frame mix of dev_ragged.py (8 each of 1920x1080, 1280x720, 1024x768, 641x359, S-text, shuffled) from host memory,
five ways in one process:
  (a) back-to-back str_er_detect_bgr_list calls on the host frames (pageable staging inside the call);
  (b) a depth-3 str_er_stream fed with str_er_stream_submit_copy_list;
  (c) a depth-3 stream, the frames written straight into the acquired staging buffer (--writers threads, as decoders would) + submit_list;
  (d) the list call on device-resident frames (the ceiling: no host link, no host copy);
  (e) (c) with the frames as NV12 (submit_nv12_list).
Rounds alternate the order of the ways; each timed region runs >= --min-s seconds (whole lists, the stream drained inside the region);
frames/s = median over --rounds rounds.  host_write_ms: the median time of (c)'s / (e)'s writes of one list into a buffer, alone.

    python tools/dev_ragged_stream.py --config pyr3x8|native6 [--out profiles/ragged_stream_<config>.json]
    python tools/dev_ragged_stream.py --config pyr3x8 --nv12-kernels 5   # NV12 list vs uniform NV12 calls on the same pixels, no timing
                                                                         # (for a rocprofv3 --kernel-trace --stats run)
"""
import argparse, json, os, sys, tempfile, time
from concurrent.futures import ThreadPoolExecutor
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S  # noqa: E402

SIZES = [(1920, 1080), (1280, 720), (1024, 768), (641, 359)]
NV12_SIZES = [(1920, 1080), (1280, 720), (1024, 768), (640, 360)]      # (NV12: even sizes; 641 x 359 -> 640 x 360)
CONFIGS = {"pyr3x8": dict(n_pyr_levels=8, channel_mask=0x07), "native6": dict(n_pyr_levels=1, channel_mask=0x3F)}
DEPTH = 3


def mix(sizes, seed_base=0):
    frames = [S.synth.stext_bgr(S.synth.frame_seed(seed_base + 100 * k + i), w, h) for k, (w, h) in enumerate(sizes) for i in range(8)]
    order = np.random.default_rng(7).permutation(len(frames))
    return [frames[i] for i in order]


def layout_of(frames, bpp_rows):
    """Tight layout, each frame from a 4-byte boundary: [(offset, w, h, stride)]."""
    lay, at = [], 0
    for fr in frames:
        rows, row, w, h = bpp_rows(fr)
        at = (at + 3) & ~3
        lay.append((at, w, h, row))
        at += rows * row
    return lay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="pyr3x8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.5)
    ap.add_argument("--writers", type=int, default=4)
    ap.add_argument("--nv12-kernels", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(); sp, wp = S.cascade_io.write_golden(tmp)
    prm = S.Params(max_width=1920, max_height=1080, max_frames=32, **CONFIGS[a.config])
    f = S.ERFilter(params=prm)
    f.load_cascade(0, sp); f.load_cascade(1, wp)
    frames = mix(SIZES)
    nv = [S.synth.nv12_from_bgr(b) for b in mix(NV12_SIZES)]

    if a.nv12_kernels:
        groups = {}
        for n in nv:
            groups.setdefault(n.shape, []).append(n)
        for _ in range(a.nv12_kernels):
            n_l = len(f.text_detect_nv12_list(nv).cands)
            n_u = sum(len(f.text_detect_nv12(np.stack(g), g[0].shape[1], g[0].shape[0] // 3 * 2).cands) for g in groups.values())
        print(json.dumps({"config": a.config, "nv12_kernels": a.nv12_kernels, "cands_list": n_l, "cands_uniform": n_u}))
        return

    bgr_lay = layout_of(frames, lambda fr: (fr.shape[0], 3 * fr.shape[1], fr.shape[1], fr.shape[0]))
    nv_lay = layout_of(nv, lambda n: (n.shape[0], n.shape[1], n.shape[1], n.shape[0] // 3 * 2))
    pool = ThreadPoolExecutor(a.writers)
    st = S.FrameStream(prm, depth=DEPTH)
    st.load_cascade(0, sp); st.load_cascade(1, wp)
    dev = [torch.from_numpy(np.ascontiguousarray(fr).reshape(-1)).cuda() for fr in frames]
    torch.cuda.synchronize()
    dev_refs = [(t.data_ptr(), fr.shape[1], fr.shape[0]) for t, fr in zip(dev, frames)]

    def write(buf, lay, srcs):
        list(pool.map(lambda k: buf.__setitem__(slice(lay[k][0], lay[k][0] + srcs[k].size), srcs[k].reshape(-1)), range(len(srcs))))

    def region(submit_one, min_s):
        """Whole lists through the stream for >= min_s, drained inside the region: (lists, seconds, candidates of the first)."""
        n, cands, t0 = 0, None, time.perf_counter()
        while True:
            if st.pending() == DEPTH:
                _, r = st.next()
                cands = len(r.cands) if cands is None else cands
            submit_one(); n += 1
            if time.perf_counter() - t0 >= min_s:
                break
        while st.pending():
            _, r = st.next()
            cands = len(r.cands) if cands is None else cands
        return n, time.perf_counter() - t0, cands

    def sub_copy():
        st.submit_copy_list(frames)

    def sub_direct():
        slot, buf = st.acquire()
        write(buf, bgr_lay, frames)
        st.submit_list(slot, bgr_lay)

    def sub_nv12():
        slot, buf = st.acquire()
        write(buf, nv_lay, nv)
        st.submit_nv12_list(slot, nv_lay)

    def call_region(fn, min_s):
        n, cands, t0 = 0, None, time.perf_counter()
        while True:
            c = fn(); n += 1
            cands = c if cands is None else cands
            if time.perf_counter() - t0 >= min_s:
                break
        return n, time.perf_counter() - t0, cands

    ways = {"a_list_call": lambda m: call_region(lambda: len(f.text_detect_list(frames).cands), m),
            "b_stream_copy_list": lambda m: region(sub_copy, m),
            "c_stream_direct": lambda m: region(sub_direct, m),
            "d_device_list": lambda m: call_region(lambda: len(f.detect_bgr_list_device(dev_refs).cands), m),
            "e_stream_nv12": lambda m: region(sub_nv12, m)}
    cands = {k: fn(0.0)[2] for k, fn in ways.items()}          # (warm-up: one list each; and the BGR ways find the same candidates)
    assert len({cands[k] for k in ("a_list_call", "b_stream_copy_list", "c_stream_direct", "d_device_list")}) == 1, cands
    fps = {k: [] for k in ways}
    names = list(ways)
    for r in range(a.rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            n, dt, _ = ways[name](a.min_s)
            fps[name].append(n * len(frames) / dt)
    wt = {"bgr": [], "nv12": []}
    slot, buf = st.acquire()
    for _ in range(9):
        for k, (lay, srcs) in (("bgr", (bgr_lay, frames)), ("nv12", (nv_lay, nv))):
            t0 = time.perf_counter(); write(buf, lay, srcs); wt[k].append(1e3 * (time.perf_counter() - t0))
    st.close()
    med = {k: float(np.median(v)) for k, v in fps.items()}
    out = {"config": a.config, "frames": len(frames), "sizes": SIZES, "nv12_sizes": NV12_SIZES, "depth": DEPTH, "writers": a.writers,
           "rounds": a.rounds, "min_s": a.min_s, "cands": cands, "list_bytes_bgr": int(sum(fr.size for fr in frames)),
           "list_bytes_nv12": int(sum(n.size for n in nv)), "frames_per_s_median": med, "frames_per_s_all": fps,
           "host_write_ms_median": {k: float(np.median(v)) for k, v in wt.items()},
           "c_over_d": med["c_stream_direct"] / med["d_device_list"], "c_over_a": med["c_stream_direct"] / med["a_list_call"],
           "b_over_a": med["b_stream_copy_list"] / med["a_list_call"], "e_over_d": med["e_stream_nv12"] / med["d_device_list"]}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
