#!/usr/bin/env python3
"""Developer aid: what the lexicon matcher (STR_ER_WANT_WORD_MATCH, str_er_match_words) costs (profiles/word_match.md).

    python tools/dev_word_match.py kernel [--words 1000] [--entries 100000] [--reps 7] [--host-words 100] [--iters N]
        match_words on random words against a random lexicon (m and l drawn from 3 .. 12, band 2): the time of every call (upload,
        k_word_match, k_word_match_final, copy back, wait), and the single-thread time of the host rules (str_er_match_words_host) on the
        first --host-words words of the same input, with the records compared.  --iters: calls only, for a
        `rocprofv3 --kernel-trace --stats` run, which gives the kernel time.  STR_ER_LIB loads another build (the other LDS layout).
    python tools/dev_word_match.py detect [--root DIR] [--reps 40] [--match]
        the detect call of tests/test_word_match_pipeline.py (two 640 x 480 S-text frames, two pyramid levels, grouped stages, masks,
        frame lines, line words, run reading): every call time, median, minimum, maximum.  --root runs another checkout (the parent),
        --match adds the flag and prints how many words take an entry other than their reading.
"""
import argparse, gzip, json, os, sys, tempfile, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["kernel", "detect"])
ap.add_argument("--words", type=int, default=1000)
ap.add_argument("--entries", type=int, default=100000)
ap.add_argument("--host-words", type=int, default=100)
ap.add_argument("--reps", type=int, default=0)
ap.add_argument("--iters", type=int, default=0)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--match", action="store_true")
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
    words = ["".join(letters[rng.integers(0, 65, int(l))]) for l in rng.integers(3, 13, a.entries)]
    n_of = rng.integers(3, 13, a.words).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]]).astype(np.int32)
    costs = rng.integers(40, 256, (int(n_of.sum()), 65))
    cheap = rng.random(costs.shape) < 0.05
    costs[cheap] = rng.integers(0, 16, int(cheap.sum()))
    costs = costs.astype(np.uint8)
    f = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    f.set_lexicon(words)
    f.set_word_match(64, 64, 2)
    out = {"lib": S.lib_path(), "words": a.words, "entries": a.entries, "lexicon": f.lexicon_info()}
    got = f.match_words(costs, first, n_of)
    out["tried"] = int(got["n_tried"].astype(np.int64).sum())
    cells = 0
    lens = np.bincount([len(w) for w in words], minlength=33)
    for m in n_of:
        for l in range(max(1, m - 2), min(32, m + 2) + 1):
            cells += int(lens[l]) * int(m) * l
    out["dp_cells"] = cells
    if a.iters:
        for _ in range(a.iters):
            f.match_words(costs, first, n_of)
        out["iters"] = a.iters
    else:
        t = []
        for _ in range(a.reps or 7):
            t0 = time.perf_counter()
            f.match_words(costs, first, n_of)
            t.append((time.perf_counter() - t0) * 1e3)
        out["match_words_call_ms"] = stats(t)
        hw = min(a.host_words, a.words)
        t0 = time.perf_counter()
        host = S.match_words_host(costs, first[:hw], n_of[:hw], words, True, 64, 64, 2)
        dt = time.perf_counter() - t0
        assert host.tobytes() == got[:hw].tobytes()
        out["host_one_thread"] = {"words": hw, "ms": round(dt * 1e3, 1), "ms_scaled_to_all_words": round(dt * 1e3 * a.words / hw, 1)}
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
    out = {"root": os.path.abspath(a.root), "lib": S.lib_path(), "match": a.match, "lines": len(plain.texts), "runs": len(plain.line_runs), "words": len(plain.words)}
    if a.match:
        rng = np.random.default_rng(9)
        read = sorted({plain.word_text(w) for w in range(len(plain.words))})
        read = [t for t in read if 1 <= len(t) <= 32]
        lexicon = read + ["".join(rng.choice(list(ALPHABET), int(rng.integers(1, 13)))) for _ in range(300)]
        f.set_lexicon(lexicon)
        flags |= S.WANT_WORD_MATCH
        r = f.text_detect(frames, flags)
        same = sum(r.word_match_text(w) == r.word_text(w) for w in range(len(r.words)))
        out.update(lexicon=len(lexicon), words_matching_their_reading=same, words_matching_their_reading_under_fold=sum(
            r.word_match_text(w).lower() == r.word_text(w).lower() for w in range(len(r.words))),
            words_without_a_match=int((r.word_matches["entry"] < 0).sum()))
        f.set_lexicon(lexicon[len(read):])
        r2 = f.text_detect(frames, flags)
        out["distractors_only"] = {"words_with_a_match": int((r2.word_matches["entry"] >= 0).sum()),
                                   "median_cost_over_free_cost": float(np.median((r2.word_matches["cost"] - r2.word_matches["free_cost"])[r2.word_matches["entry"] >= 0]))}
        f.set_lexicon(lexicon)
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
