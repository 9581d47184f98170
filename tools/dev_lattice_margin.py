#!/usr/bin/env python3
"""Developer aid: what the lattice decoder's margins (str_er_set_lattice_margin, str_er_lattice_margins) cost (profiles/lattice_margin.md).

    python tools/dev_lattice_margin.py kernel [--words 1000] [--cuts none|random] [--ins 0] [--del 0] [--reps 7] [--iters N] [--edges] [--marginals]
        lattice_margins on the workload of tools/dev_lattice_decode.py kernel (its 1000 words of 3 .. 12 runs, every run uncut or given
        1 .. 3 cuts with random piece rows, the same table): the time of every call (upload, k_lattice_decode, k_lattice_margin, copy
        back, wait) beside that of lattice_decode_words, and the single-thread time of the host rules (str_er_lattice_margins_host) on
        the same input, with the tables compared.  --iters: calls only, for a `rocprofv3 --kernel-trace --stats` run, which gives the
        two kernels' times side by side.
    python tools/dev_lattice_margin.py detect [--root DIR] [--reps 40] [--margin] [--ins 0] [--del 0]
        the detect call of tools/dev_lattice_decode.py detect --lattice (two 640 x 480 S-text frames, two pyramid levels, grouped stages,
        masks, frame lines, line words, run reading, run split, lattice decode): every call time, median, minimum, maximum.  --root runs
        another checkout (the parent, which has no setting: --margin must be left out), --margin switches the setting on and prints how
        the margins of the call's words spread.
"""
import argparse, gzip, json, os, sys, tempfile, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["kernel", "detect"])
ap.add_argument("--words", type=int, default=1000)
ap.add_argument("--cuts", choices=["none", "random"], default="random")
ap.add_argument("--reps", type=int, default=0)
ap.add_argument("--iters", type=int, default=0)
ap.add_argument("--ins", type=int, default=0)
ap.add_argument("--del", dest="dele", type=int, default=0)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--margin", action="store_true")
ap.add_argument("--edges", action="store_true")
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


def rows_like(rng, n):
    costs = rng.integers(40, 256, (n, 65))
    cheap = rng.random(costs.shape) < 0.05
    costs[cheap] = rng.integers(0, 16, int(cheap.sum()))
    return costs.astype(np.uint8)


def kernel():
    rng = np.random.default_rng(1)                                       # (the draws of dev_lattice_decode.py kernel, in its order: the same table, words, cuts and rows)
    letters = np.array(list(ALPHABET))
    table = S.bigram_from_words(["".join(letters[rng.integers(0, 65, int(l))]) for l in rng.integers(3, 13, 2000)])
    n_of = rng.integers(3, 13, a.words).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(n_of)])[:a.words].astype(np.int32)
    costs = rows_like(rng, int(n_of.sum()))
    sp = np.zeros(len(costs), S.RUN_SPLIT_DTYPE)
    sp["cut"] = -1
    sp["n_cuts"] = rng.integers(1, 4, len(costs)) if a.cuts == "random" else 0
    sp["n_pieces"] = np.where(sp["n_cuts"] > 0, (sp["n_cuts"] + 1) * (sp["n_cuts"] + 2) // 2 - 1, 0)
    sp["first_piece"] = np.concatenate([[0], np.cumsum(sp["n_pieces"])])[:len(sp)]
    pieces = rows_like(rng, int(sp["n_pieces"].sum()))
    atoms = np.array([int((sp["n_cuts"][f:f + k] + 1).sum()) for f, k in zip(first, n_of)], np.int32)
    f = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    f.set_bigram(table)
    f.set_word_decode(a.ins, a.dele)
    out = {"lib": S.lib_path(), "words": a.words, "runs": int(n_of.sum()), "cuts": a.cuts, "pieces": len(pieces), "atoms": int(atoms.sum()),
           "words_over_32_atoms": int((atoms > 32).sum()), "ins": a.ins, "del": a.dele, "edges": a.edges, "marginals": a.marginals}
    call = lambda: f.lattice_margins(sp, costs, pieces, first, n_of, want_edges=a.edges, want_marginals=a.marginals)
    got = call()
    rec = got[0]
    rm, cm = rec["read_margin"].astype(np.int64), rec["cut_margin"].astype(np.int64)
    out["margins"] = {"not_decoded": int((rm < 0).sum()), "edges": int(rec["n_edges"].sum()), "read_zero": int((rm == 0).sum()),
                      "read_median": float(np.median(rm[rm >= 0])) if (rm >= 0).any() else None, "words_with_a_cut_margin": int((cm >= 0).sum()),
                      "cut_zero": int((cm == 0).sum()), "cut_median": float(np.median(cm[cm >= 0])) if (cm >= 0).any() else None,
                      "parts_read_as_dropped": int((got[3] == 65).sum())}
    if a.iters:
        for _ in range(a.iters):
            call()
        out["iters"] = a.iters
    else:
        reps = a.reps or 7
        out["lattice_margins_call_ms"] = timed(call, reps)
        out["lattice_decode_words_call_ms"] = timed(lambda: f.lattice_decode_words(sp, costs, pieces, first, n_of), reps)
        t0 = time.perf_counter()
        host = S.lattice_margins_host(sp, costs, pieces, first, n_of, table, a.ins, a.dele, 8, want_edges=a.edges, want_marginals=a.marginals)
        dt = time.perf_counter() - t0
        assert all(h is None and g is None or h.tobytes() == g.tobytes() for h, g in zip(host, got))
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
    f.set_run_split(1, 2, 8)
    flags |= S.WANT_RUN_SPLIT | S.WANT_LATTICE_DECODE
    if a.margin:
        f.set_lattice_margin(True)
        r = f.text_detect(frames, flags)
        rm, cm = r.lattice_margins["read_margin"].astype(np.int64), r.lattice_margins["cut_margin"].astype(np.int64)
        out["margins"] = {"not_decoded": int((rm < 0).sum()), "read_zero": int((rm == 0).sum()), "read_median": float(np.median(rm[rm >= 0])) if (rm >= 0).any() else None,
                          "words_with_a_cut_margin": int((cm >= 0).sum()), "cut_zero": int((cm == 0).sum()),
                          "cut_median": float(np.median(cm[cm >= 0])) if (cm >= 0).any() else None}
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
