#!/usr/bin/env python3
"""Developer aid: what the splitting of touching glyphs (STR_ER_WANT_RUN_SPLIT, str_er_feet_split, str_er_split_words) costs
(profiles/run_split.md).

    python tools/dev_run_split.py kernel [--lines 400] [--words 1000] [--reps 7] [--iters N]
        feet_split (cuts and pieces alone: k_foot_words, k_run_cuts, k_run_tiles and the feature kernels) on footprints of two to
        four lobes joined by necks, and split_words on random cost rows of words of 3 .. 12 runs with 0 .. 3 cuts a run: the time of
        every call, the host rules (str_er_split_words_host) on one thread with the tables compared.  --iters: calls only, for a
        `rocprofv3 --kernel-trace --stats` run, which gives the times of k_run_cuts and k_split_words.
    python tools/dev_run_split.py detect [--root DIR] [--reps 40] [--split] [--decode]
        the detect call of tests/test_run_split_pipeline.py (two 640 x 480 S-text frames, two pyramid levels, grouped stages, masks,
        frame lines, line words, run reading): every call time, median, minimum, maximum.  --root runs another checkout (the parent,
        without --split), --split adds the flag (valley threshold 1 / 2) and prints the counts, --decode the bigram decoder as well.
"""
import argparse, gzip, json, os, sys, tempfile, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["kernel", "detect"])
ap.add_argument("--lines", type=int, default=400)
ap.add_argument("--words", type=int, default=1000)
ap.add_argument("--reps", type=int, default=0)
ap.add_argument("--iters", type=int, default=0)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--split", action="store_true")
ap.add_argument("--decode", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import torch  # noqa: F401,E402  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S  # noqa: E402

ALPHABET = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz&()"


def stats(t):
    return {"calls": [round(x, 3) for x in t], "median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def timed(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return stats(t)


def lobed(rng, h, lobes):
    """A footprint of one run: lobes of 4 .. 24 columns (every column above h / 4) joined by necks of 1 .. 3 columns of one pixel."""
    cols = []
    for k in range(lobes):
        if k:
            cols += [1] * int(rng.integers(1, 4))
        cols += [int(v) for v in rng.integers(h // 4 + 1, h + 1, int(rng.integers(4, 25)))]
    b = np.zeros((h, len(cols)), bool)
    for c, v in enumerate(cols):
        b[rng.permutation(h)[:v], c] = True
    b[0, 0] = b[h - 1, 0] = True
    return b


def kernel():
    rng = np.random.default_rng(1)
    W, H = 1920, 1080
    feet, words = np.zeros(a.lines, S.LINE_FOOT_DTYPE), []
    for t in range(a.lines):
        b = lobed(rng, int(rng.integers(12, 49)), int(rng.integers(2, 5)))
        h, w = b.shape
        feet[t]["x"], feet[t]["y"], feet[t]["w"], feet[t]["h"], feet[t]["pixels"] = int(rng.integers(0, W - w)), int(rng.integers(0, H - h)), w, h, int(b.sum())
        bits = np.zeros((h, (w + 31) // 32 * 32), bool)
        bits[:, :w] = b
        words.append(np.packbits(bits.reshape(h, -1, 32), axis=2, bitorder="little").view("<u4").reshape(-1))          # (bit i of word k: column 32 k + i)
    words = np.concatenate(words)
    f = S.ERFilter(params=S.Params(max_width=W, max_height=H, max_frames=1))
    got = f.feet_split(W, H, feet, words, None, want_reads=False, want_q=False)
    out = {"lib": S.lib_path(), "lines": a.lines, "runs": len(got["runs"]), "cut_runs": int((got["splits"]["n_cuts"] > 0).sum()), "pieces": len(got["pieces"])}
    # split_words: words of 3 .. 12 runs, 0 .. 3 cuts a run, 5 % of the characters cheap
    n_of = rng.integers(3, 13, a.words).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(n_of)])[:a.words].astype(np.int32)
    n = int(n_of.sum())
    sp = np.zeros(n, S.RUN_SPLIT_DTYPE)
    sp["cut"] = -1
    sp["n_cuts"] = rng.integers(0, 4, n)
    sp["n_pieces"] = np.where(sp["n_cuts"] > 0, (sp["n_cuts"] + 1) * (sp["n_cuts"] + 2) // 2 - 1, 0)
    sp["first_piece"] = np.concatenate([[0], np.cumsum(sp["n_pieces"])[:-1]])

    def rows(k):
        c = rng.integers(40, 256, (k, 65))
        cheap = rng.random(c.shape) < 0.05
        c[cheap] = rng.integers(0, 16, int(cheap.sum()))
        return c.astype(np.uint8)
    rc, pc = rows(n), rows(int(sp["n_pieces"].sum()))
    ws, parts, prow = f.split_words(sp, rc, pc, first, n_of)
    out.update(words=a.words, word_runs=n, word_pieces=len(pc), parts=len(parts), words_with_more_parts_than_runs=int((ws["n_parts"] > n_of).sum()))
    if a.iters:
        for _ in range(a.iters):
            f.feet_split(W, H, feet, words, None, want_reads=False, want_q=False)
            f.split_words(sp, rc, pc, first, n_of)
        out["iters"] = a.iters
    else:
        out["feet_split_call_ms"] = timed(lambda: f.feet_split(W, H, feet, words, None, want_reads=False, want_q=False), a.reps or 7)
        out["feet_read_call_ms"] = timed(lambda: f.feet_read(W, H, feet, words, None, want_reads=False), a.reps or 7)
        out["split_words_call_ms"] = timed(lambda: f.split_words(sp, rc, pc, first, n_of), a.reps or 7)
        t0 = time.perf_counter()
        hw, hp, hr = S.split_words_host(sp, rc, pc, first, n_of, 8)
        out["host_one_thread_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        assert hw.tobytes() == ws.tobytes() and hp.tobytes() == parts.tobytes() and hr.tobytes() == prow.tobytes()
    f.close()
    return out


def detect():
    tmp = tempfile.mkdtemp(); sp, wp = S.cascade_io.write_golden(tmp)
    model = os.path.join(tmp, "ocr.model")
    with open(model, "wb") as fh:
        fh.write(gzip.open(S.cascade_io.ocr_model_path(5)).read())
    sy = S.synth
    frames = np.stack([sy.stext_bgr(sy.frame_seed(2), 640, 480), sy.stext_bgr(sy.frame_seed(976), 640, 480)])
    f = S.ERFilter(params=S.Params(max_width=640, max_height=480, max_frames=2, n_pyr_levels=2))
    f.load_cascade(0, sp); f.load_cascade(1, wp)
    f.load_svm_model(model, 1800)
    flags = S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP | S.WANT_MASKS | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS | S.WANT_RUN_READ
    plain = f.text_detect(frames, flags)
    out = {"root": os.path.abspath(a.root), "lib": S.lib_path(), "split": a.split, "decode": a.decode, "lines": len(plain.texts), "runs": len(plain.line_runs),
           "words": len(plain.words)}
    if a.decode:
        read = sorted({plain.word_text(w) for w in range(len(plain.words))})
        f.set_bigram(S.bigram_from_words([t for t in read if t and all(ch in ALPHABET for ch in t)]))
        flags |= S.WANT_WORD_DECODE
    if a.split:
        f.set_run_split(1, 2, 8)
        flags |= S.WANT_RUN_SPLIT
        r = f.text_detect(frames, flags)
        out.update(cut_runs=int((r.run_splits["n_cuts"] > 0).sum()), pieces=len(r.run_pieces), parts=len(r.split_parts),
                   words_with_more_parts_than_runs=int((r.word_splits["n_parts"] > r.words["n_runs"]).sum()))
    for _ in range(5):
        f.text_detect(frames, flags)
    out["detect_call_ms"] = timed(lambda: f.text_detect(frames, flags), a.reps or 40)
    f.close()
    return out


if __name__ == "__main__":
    res = kernel() if a.mode == "kernel" else detect()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
