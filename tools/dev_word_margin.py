#!/usr/bin/env python3
"""Developer aid: what the word decoder's margins (str_er_set_word_margin, str_er_word_margins) cost (profiles/word_margin.md).

    python tools/dev_word_margin.py kernel [--words 1000] [--reps 7] [--ins 0] [--del 0] [--iters N] [--marginals]
        word_margins on the workload of tools/dev_word_decode.py kernel (random words of 3 .. 12 runs under a table from random words):
        the time of every call (upload, k_word_decode, k_word_margin, copy back, wait) beside that of decode_words, and the
        single-thread time of the host rules (str_er_word_margins_host) on the same input, with the tables compared.  --iters: calls
        only, for a `rocprofv3 --kernel-trace --stats` run, which gives the two kernels' times side by side.
    python tools/dev_word_margin.py detect [--root DIR] [--reps 40] [--margin] [--ins 0] [--del 0]
        the detect call of tests/test_word_margin_pipeline.py (two 640 x 480 S-text frames, two pyramid levels, grouped stages, masks,
        frame lines, line words, run reading, word decode): every call time, median, minimum, maximum.  --root runs another checkout
        (the parent, which has no setting: --margin must be left out), --margin switches the setting on and prints how the margins
        of the call's words spread.
"""
import argparse, gzip, json, os, sys, tempfile, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["kernel", "detect"])
ap.add_argument("--words", type=int, default=1000)
ap.add_argument("--reps", type=int, default=0)
ap.add_argument("--iters", type=int, default=0)
ap.add_argument("--ins", type=int, default=0)
ap.add_argument("--del", dest="dele", type=int, default=0)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--margin", action="store_true")
ap.add_argument("--marginals", action="store_true")
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


def kernel():
    rng = np.random.default_rng(1)                       # (the words, rows and table of tools/dev_word_decode.py kernel)
    letters = np.array(list(ALPHABET))
    table = S.bigram_from_words(["".join(letters[rng.integers(0, 65, int(l))]) for l in rng.integers(3, 13, 2000)])
    n_of = rng.integers(3, 13, a.words).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(n_of)])[:a.words].astype(np.int32)
    costs = rng.integers(40, 256, (int(n_of.sum()), 65))
    cheap = rng.random(costs.shape) < 0.05
    costs[cheap] = rng.integers(0, 16, int(cheap.sum()))
    costs = costs.astype(np.uint8)
    f = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    f.set_bigram(table)
    f.set_word_decode(a.ins, a.dele)
    out = {"lib": S.lib_path(), "words": a.words, "runs": int(n_of.sum()), "ins": a.ins, "del": a.dele, "marginals": a.marginals}
    rec, rm, rr, ra, mg = f.word_margins(costs, first, n_of, want_marginals=a.marginals)
    m = rec["margin"].astype(np.int64)
    out["margin"] = {"zero": int((m == 0).sum()), "median": float(np.median(m)), "max": int(m.max()), "rows_read_as_dropped": int((rr == 65).sum()),
                     "rows_whose_alternative_is_the_drop": int((ra == 65).sum())}
    if a.iters:
        for _ in range(a.iters):
            f.word_margins(costs, first, n_of, want_marginals=a.marginals)
        out["iters"] = a.iters
    else:
        reps = a.reps or 7
        out["word_margins_call_ms"] = timed(lambda: f.word_margins(costs, first, n_of, want_marginals=a.marginals), reps)
        out["decode_words_call_ms"] = timed(lambda: f.decode_words(costs, first, n_of), reps)
        t0 = time.perf_counter()
        host = S.word_margins_host(costs, first, n_of, table, a.ins, a.dele, want_marginals=a.marginals)
        dt = time.perf_counter() - t0
        assert host[0].tobytes() == rec.tobytes() and host[1].tobytes() == rm.tobytes() and host[2].tobytes() == rr.tobytes() and host[3].tobytes() == ra.tobytes()
        assert mg is None or host[4].tobytes() == mg.tobytes()
        out["host_one_thread_ms"] = round(dt * 1e3, 2)
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
    out = {"root": os.path.abspath(a.root), "lib": S.lib_path(), "margin": a.margin, "ins": a.ins, "dele": a.dele, "lines": len(plain.texts),
           "runs": len(plain.line_runs), "words": len(plain.words)}
    read = sorted({plain.word_text(w) for w in range(len(plain.words))})
    f.set_bigram(S.bigram_from_words([t for t in read if t and all(ch in ALPHABET for ch in t)]))
    f.set_word_decode(a.ins, a.dele)
    flags |= S.WANT_WORD_DECODE
    if a.margin:
        f.set_word_margin(True)
        m = f.text_detect(frames, flags).word_margins["margin"].astype(np.int64)
        out["margins"] = {"not_decoded": int((m < 0).sum()), "zero": int((m == 0).sum()), "median": float(np.median(m[m >= 0])) if (m >= 0).any() else None,
                          "max": int(m.max(initial=-1))}
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
