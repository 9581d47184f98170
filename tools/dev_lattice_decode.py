#!/usr/bin/env python3
"""Developer aid: what the joint decode over the piece lattice (STR_ER_WANT_LATTICE_DECODE, str_er_lattice_decode_words) costs
(profiles/lattice_decode.md).

    python tools/dev_lattice_decode.py kernel [--words 1000] [--cuts none|random] [--ins 0] [--del 0] [--reps 7]
                                              [--iters N --what lattice|decode_runs|split_decode|decode_atoms]
        tools/dev_word_decode.py's 1000 words of 3 .. 12 runs (the same rows, the same table), every run uncut or given 1 .. 3 cuts with
        random piece rows: the time of every lattice_decode_words call (upload, k_lattice_decode, copy back, wait) and the single-thread
        time of the host rules (str_er_lattice_decode_words_host) on the same input, with the tables compared.  --iters: calls only, for a
        `rocprofv3 --kernel-trace --stats` run, which gives the kernel times; --what picks the calls: the lattice decode, decode_words on
        the runs' rows (k_word_decode on the same rows), split_words and decode_words on its parts (k_split_words + k_word_decode), or
        decode_words on sequences of N rows, N the atoms of every word (k_word_decode alone on as many products).
    python tools/dev_lattice_decode.py detect [--root DIR] [--reps 40] [--lattice] [--ins 0] [--del 0]
        the detect call of the pipeline tests (two 640 x 480 S-text frames, two pyramid levels, grouped stages, masks, frame lines, line
        words, run reading): every call time, median, minimum, maximum.  --root runs another checkout (the parent), --lattice adds
        STR_ER_WANT_RUN_SPLIT and the flag and prints what the lattice decode made of the words.
"""
import argparse, gzip, json, os, sys, tempfile, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["kernel", "detect"])
ap.add_argument("--words", type=int, default=1000)
ap.add_argument("--cuts", choices=["none", "random"], default="random")
ap.add_argument("--what", choices=["lattice", "decode_runs", "split_decode", "decode_atoms"], default="lattice")
ap.add_argument("--reps", type=int, default=0)
ap.add_argument("--iters", type=int, default=0)
ap.add_argument("--ins", type=int, default=0)
ap.add_argument("--del", dest="dele", type=int, default=0)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--lattice", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import torch  # noqa: F401,E402  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S  # noqa: E402

ALPHABET = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz&()"


def stats(t):
    return {"calls": [round(x, 3) for x in t], "median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def rows_like(rng, n):
    costs = rng.integers(40, 256, (n, 65))
    cheap = rng.random(costs.shape) < 0.05
    costs[cheap] = rng.integers(0, 16, int(cheap.sum()))
    return costs.astype(np.uint8)


def kernel():
    rng = np.random.default_rng(1)                                       # (the draws of dev_word_decode.py, in its order: the same table, words and rows)
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
           "words_over_32_atoms": int((atoms > 32).sum()), "ins": a.ins, "del": a.dele}
    dec, chars, src, parts = f.lattice_decode_words(sp, costs, pieces, first, n_of)
    ok = dec["cost"] >= 0
    out["moves"] = {k: int(dec[k].astype(np.int64).sum()) for k in ("n_sub", "n_del", "n_ins", "n_parts")}
    out["parts_that_are_pieces"] = int((parts["piece"] >= 0).sum())
    out["words_cheaper_than_their_reading"] = int((dec["cost"] < dec["read_cost"])[ok].sum())
    if a.iters:
        atom_first = np.concatenate([[0], np.cumsum(atoms)])[:a.words].astype(np.int32)
        atom_rows = rows_like(rng, int(atoms.sum()))
        for _ in range(a.iters):
            if a.what == "lattice":
                f.lattice_decode_words(sp, costs, pieces, first, n_of)
            elif a.what == "decode_runs":
                f.decode_words(costs, first, n_of)
            elif a.what == "split_decode":
                ws, _, prow = f.split_words(sp, costs, pieces, first, n_of)
                f.decode_words(prow, ws["first_part"], ws["n_parts"])
            else:
                f.decode_words(atom_rows, atom_first, atoms)
        out["iters"], out["what"] = a.iters, a.what
    else:
        t = []
        for _ in range(a.reps or 7):
            t0 = time.perf_counter()
            f.lattice_decode_words(sp, costs, pieces, first, n_of)
            t.append((time.perf_counter() - t0) * 1e3)
        out["lattice_decode_words_call_ms"] = stats(t)
        t0 = time.perf_counter()
        hd, hc, hs, hp = S.lattice_decode_words_host(sp, costs, pieces, first, n_of, table, a.ins, a.dele, 8)
        dt = time.perf_counter() - t0
        assert hd.tobytes() == dec.tobytes() and hc.tobytes() == chars.tobytes() and hs.tobytes() == src.tobytes() and hp.tobytes() == parts.tobytes()
        out["host_one_thread_ms"] = round(dt * 1e3, 2)
        out["lattice_decode_table_bytes"] = f.lattice_decode_stats()
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
    out = {"root": os.path.abspath(a.root), "lib": S.lib_path(), "lattice": a.lattice, "lines": len(plain.texts), "runs": len(plain.line_runs), "words": len(plain.words)}
    if a.lattice:
        read = sorted({plain.word_text(w) for w in range(len(plain.words))})
        f.set_bigram(S.bigram_from_words([t for t in read if t and all(ch in ALPHABET for ch in t)]))
        f.set_word_decode(a.ins, a.dele)
        f.set_run_split(1, 2, 8)
        flags |= S.WANT_RUN_SPLIT | S.WANT_LATTICE_DECODE
        r = f.text_detect(frames, flags)
        d = r.lattice_decodes
        out.update(ins=a.ins, dele=a.dele, cut_runs=int((r.run_splits["n_cuts"] > 0).sum()), pieces=len(r.run_pieces),
                   words_keeping_their_reading=sum(r.word_lattice_text(w) == r.word_text(w) for w in range(len(r.words))),
                   words_not_decoded=int((d["cost"] < 0).sum()), parts=int(d["n_parts"].sum()), parts_that_are_pieces=int((r.lattice_parts["piece"] >= 0).sum()),
                   parts_dropped=int(d["n_del"].sum()), characters_inserted=int(d["n_ins"].sum()))
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
