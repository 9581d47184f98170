#!/usr/bin/env python3
"""Developer aid: what the word decoder (STR_ER_WANT_WORD_DECODE, str_er_decode_words) costs (profiles/word_decode.md).

    python tools/dev_word_decode.py kernel [--words 1000] [--reps 7] [--ins 0] [--del 0] [--iters N]
        decode_words on random words of 3 .. 12 runs under a table from random words: the time of every call (upload, k_word_decode,
        copy back, wait), and the single-thread time of the host rules (str_er_decode_words_host) on the same input, with the tables
        compared.  --iters: calls only, for a `rocprofv3 --kernel-trace --stats` run, which gives the kernel time.  STR_ER_LIB loads
        another build (the other way of reading the predecessors: -DWD_READLANE=1).
    python tools/dev_word_decode.py detect [--root DIR] [--reps 40] [--decode] [--ins 0] [--del 0]
        the detect call of tests/test_word_decode_pipeline.py (two 640 x 480 S-text frames, two pyramid levels, grouped stages, masks,
        frame lines, line words, run reading): every call time, median, minimum, maximum.  --root runs another checkout (the parent),
        --decode adds the flag and prints how many words keep their reading.
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
ap.add_argument("--decode", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import torch  # noqa: F401,E402  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S  # noqa: E402

ALPHABET = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz&()"


def stats(t):
    return {"calls": [round(x, 3) for x in t], "median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def kernel():
    rng = np.random.default_rng(1)
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
    out = {"lib": S.lib_path(), "words": a.words, "runs": int(n_of.sum()), "ins": a.ins, "del": a.dele, "bigram": f.bigram_info()}
    dec, chars, src = f.decode_words(costs, first, n_of)
    out["moves"] = {k: int(dec[k].astype(np.int64).sum()) for k in ("n_sub", "n_del", "n_ins")}
    out["words_cheaper_than_their_reading"] = int((dec["cost"] < dec["read_cost"]).sum())
    if a.iters:
        for _ in range(a.iters):
            f.decode_words(costs, first, n_of)
        out["iters"] = a.iters
    else:
        t = []
        for _ in range(a.reps or 7):
            t0 = time.perf_counter()
            f.decode_words(costs, first, n_of)
            t.append((time.perf_counter() - t0) * 1e3)
        out["decode_words_call_ms"] = stats(t)
        t0 = time.perf_counter()
        hd, hc, hs = S.decode_words_host(costs, first, n_of, table, a.ins, a.dele)
        dt = time.perf_counter() - t0
        assert hd.tobytes() == dec.tobytes() and hc.tobytes() == chars.tobytes() and hs.tobytes() == src.tobytes()
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
    out = {"root": os.path.abspath(a.root), "lib": S.lib_path(), "decode": a.decode, "lines": len(plain.texts), "runs": len(plain.line_runs), "words": len(plain.words)}
    if a.decode:
        read = sorted({plain.word_text(w) for w in range(len(plain.words))})
        f.set_bigram(S.bigram_from_words([t for t in read if t and all(ch in ALPHABET for ch in t)]))
        f.set_word_decode(a.ins, a.dele)
        flags |= S.WANT_WORD_DECODE
        r = f.text_detect(frames, flags)
        d = r.word_decodes
        out.update(ins=a.ins, dele=a.dele, words_keeping_their_reading=sum(r.word_decode_text(w) == r.word_text(w) for w in range(len(r.words))),
                   words_not_decoded=int((d["cost"] < 0).sum()), runs_dropped=int(d["n_del"].sum()), characters_inserted=int(d["n_ins"].sum()))
    for _ in range(5):
        f.text_detect(frames, flags)
    t = []
    for _ in range(a.reps or 40):
        t0 = time.perf_counter()
        f.text_detect(frames, flags)
        t.append((time.perf_counter() - t0) * 1e3)
    out["detect_call_ms"] = stats(t)
    f.close()
    return out


if __name__ == "__main__":
    res = kernel() if a.mode == "kernel" else detect()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
