#!/usr/bin/env python3
"""Developer aid: what the lexicon match over the piece lattice (STR_ER_WANT_LATTICE_MATCH, str_er_lattice_match_words) costs
(profiles/lattice_match.md).

    python tools/dev_lattice_match.py kernel [--words 1000] [--entries 100000] [--cuts] [--reps 7] [--host-words 100] [--iters N] [--what lattice|match]
        lattice_match_words on random words against a random lexicon (runs and entry lengths drawn from 3 .. 12, band 2, INS = DEL =
        64, SPLIT = 8, fold): without --cuts every run is uncut and match_words on the same rows is timed in the same process (the
        yardstick: the same cells); with --cuts every run has 0 .. 3 cuts and random piece rows.  Prints every call time, the entries
        tried and the cells computed (node x character x edges into the node), and the single-thread time of the host rules
        (str_er_lattice_match_words_host) on the first --host-words words, with the records compared.  --iters: calls only (of --what),
        for a `rocprofv3 --kernel-trace --stats` run, which gives the kernel times.
    python tools/dev_lattice_match.py detect [--root DIR] [--reps 40] [--flag]
        the detect call of tests/test_run_split_pipeline.py beside the matcher (two 640 x 480 S-text frames, two pyramid levels, grouped
        stages, masks, frame lines, line words, run reading, run split, word match): every call time, median, minimum, maximum.  --root
        runs another checkout (the parent), --flag adds the lattice match and prints how many words take another entry than the matcher's.
"""
import argparse, gzip, json, os, sys, tempfile, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["kernel", "detect"])
ap.add_argument("--words", type=int, default=1000)
ap.add_argument("--entries", type=int, default=100000)
ap.add_argument("--cuts", action="store_true")
ap.add_argument("--host-words", type=int, default=100)
ap.add_argument("--reps", type=int, default=0)
ap.add_argument("--iters", type=int, default=0)
ap.add_argument("--what", choices=["lattice", "match"], default="lattice")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--flag", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import torch  # noqa: F401,E402  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S  # noqa: E402

ALPHABET = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz&()"


def stats(t):
    return {"calls": [round(x, 3) for x in t], "median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def rows(rng, n):
    c = rng.integers(40, 256, (n, 65))
    cheap = rng.random(c.shape) < 0.05
    c[cheap] = rng.integers(0, 16, int(cheap.sum()))
    return c.astype(np.uint8)


def kernel():
    rng = np.random.default_rng(1)
    letters = np.array(list(ALPHABET))
    words = ["".join(letters[rng.integers(0, 65, int(l))]) for l in rng.integers(3, 13, a.entries)]
    n_of = rng.integers(3, 13, a.words).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]]).astype(np.int32)
    rc = rows(rng, int(n_of.sum()))                           # (the rows, words and lexicon of tools/dev_word_match.py kernel: the same draws)
    cuts = rng.integers(0, 4, len(rc)) if a.cuts else np.zeros(len(rc), np.int64)
    sp = np.zeros(len(rc), S.RUN_SPLIT_DTYPE)
    sp["cut"] = -1
    sp["n_cuts"] = cuts
    sp["n_pieces"] = np.where(cuts > 0, (cuts + 1) * (cuts + 2) // 2 - 1, 0)
    sp["first_piece"] = np.concatenate([[0], np.cumsum(sp["n_pieces"])[:-1]])
    pc = rows(rng, int(sp["n_pieces"].sum()))
    f = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    f.set_lexicon(words)
    f.set_word_match(64, 64, 2)
    f.set_run_split(1, 4, 8)
    out = {"lib": S.lib_path(), "words": a.words, "entries": a.entries, "cuts": a.cuts, "lexicon": f.lexicon_info()}
    got = f.lattice_match_words(sp, rc, pc, first, n_of)
    rec = got[0]
    atoms = np.array([int((cuts[s:s + k] + 1).sum()) for s, k in zip(first, n_of)])
    out["tried"] = int(rec["n_tried"].astype(np.int64).sum())
    out["words_tried"] = int((atoms <= 32).sum())
    out["words_with_more_parts_than_runs"] = int((rec["n_parts"] > n_of).sum())
    lens = np.bincount([len(w) for w in words], minlength=33)
    cells = 0                                                  # node x character x edges into the node, over the entries tried
    for s, k, N in zip(first, n_of, atoms):
        if N > 32:
            continue
        edges = int(sum((c + 1) * (c + 2) // 2 for c in cuts[s:s + k]))
        for l in range(max(1, k - 2), min(32, N + 2) + 1):
            cells += int(lens[l]) * edges * l
    out["dp_cells"] = cells
    plain = None
    if not a.cuts:
        plain = f.match_words(rc, first, n_of)
        assert [tuple(r)[:6] for r in rec.tolist()] == [tuple(r) for r in plain.tolist()]
    if a.iters:
        for _ in range(a.iters):
            if a.what == "lattice":
                f.lattice_match_words(sp, rc, pc, first, n_of)
            else:
                f.match_words(rc, first, n_of)
        out["iters"], out["what"] = a.iters, a.what
    else:
        tl, tm = [], []
        for _ in range(a.reps or 7):                           # alternated in one process
            t0 = time.perf_counter()
            f.lattice_match_words(sp, rc, pc, first, n_of)
            tl.append((time.perf_counter() - t0) * 1e3)
            if plain is not None:
                t0 = time.perf_counter()
                f.match_words(rc, first, n_of)
                tm.append((time.perf_counter() - t0) * 1e3)
        out["lattice_match_words_call_ms"] = stats(tl)
        if tm:
            out["match_words_call_ms"] = stats(tm)
        hw = min(a.host_words, a.words)
        t0 = time.perf_counter()
        host = S.lattice_match_words_host(sp, rc, pc, first[:hw], n_of[:hw], words, True, 64, 64, 2, 8)
        dt = time.perf_counter() - t0
        n_parts = int(host[0]["n_parts"].sum())
        assert host[0].tobytes() == rec[:hw].tobytes() and host[1].tobytes() == got[1][:hw].tobytes() and host[2].tobytes() == got[2][:n_parts].tobytes()
        out["host_one_thread"] = {"words": hw, "ms": round(dt * 1e3, 1), "ms_scaled_to_all_words": round(dt * 1e3 * a.words / hw, 1)}
    out["table_bytes"] = f.lattice_match_stats()
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
    flags = S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP | S.WANT_MASKS | S.WANT_FRAME_LINES | S.WANT_LINE_WORDS | S.WANT_RUN_READ | S.WANT_RUN_SPLIT
    plain = f.text_detect(frames, flags)
    rng = np.random.default_rng(9)
    read = sorted({plain.word_text(w) for w in range(len(plain.words))} | {plain.word_split_text(w) for w in range(len(plain.words))})
    read = [t for t in read if 1 <= len(t) <= 32]
    lexicon = read + ["".join(rng.choice(list(ALPHABET), int(rng.integers(1, 13)))) for _ in range(300)]
    f.set_lexicon(lexicon)
    flags |= S.WANT_WORD_MATCH
    out = {"root": os.path.abspath(a.root), "lib": S.lib_path(), "flag": a.flag, "lines": len(plain.texts), "runs": len(plain.line_runs), "words": len(plain.words),
           "runs_with_a_cut": int((plain.run_splits["n_cuts"] > 0).sum()), "lexicon": len(lexicon)}
    if a.flag:
        flags |= S.WANT_LATTICE_MATCH
        r = f.text_detect(frames, flags)
        d, m, ws, n_of = r.lattice_matches, r.word_matches, r.word_splits, r.words["n_runs"]
        out.update(words_with_another_entry_than_the_matcher=int((d["entry"] != m["entry"]).sum()),
                   words_cheaper_than_the_split_sequence=int(((m["entry"] >= 0) & (d["cost"] < m["cost"] + 8 * (ws["n_parts"] - n_of))).sum()),
                   words_with_other_parts_than_the_split_sequence=int(sum(
                       r.word_lattice_match_parts(w).tobytes() != r.split_parts[int(ws[w]["first_part"]):int(ws[w]["first_part"]) + int(ws[w]["n_parts"])].tobytes()
                       for w in range(len(d)) if d[w]["entry"] >= 0)),
                   entries_tried=int(d["n_tried"].sum()), entries_tried_by_the_matcher=int(m["n_tried"].sum()), table_bytes=f.lattice_match_stats())
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
