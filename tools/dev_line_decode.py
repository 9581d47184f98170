#!/usr/bin/env python3
"""Developer aid: what the line decoder (str_er_set_line_decode, str_er_decode_lines) and its margins (str_er_set_line_margin,
str_er_line_margins) cost (profiles/line_decode.md, profiles/line_margin.md).

    python tools/dev_line_decode.py kernel [--lines 100] [--rows 75] [--reps 7] [--ins 0] [--del 0] [--margin] [--lattice] [--iters N]
        decode_lines on lines of --rows rows each, beside decode_words on the same rows cut into words of 3 .. 12 runs (the workload
        of tools/dev_word_decode.py kernel): the time of every call, and the single-thread time of the host rules
        (str_er_decode_lines_host) on the same input, with the tables compared.  --iters: calls only, for a
        `rocprofv3 --kernel-trace --stats` run, which gives the two kernels' times side by side.  --margin: line_margins as well
        (k_line_decode and k_line_margin in one call), its call time beside decode_lines', the host rules compared.  --lattice: the
        rows are runs of 1 .. 4 atoms with their pieces' rows, and lattice_decode_lines (k_line_lattice_decode,
        profiles/line_lattice_decode.md) decodes the same lines over them, beside decode_lines on the runs' rows; its call time, the
        host rules (str_er_lattice_decode_lines_host) on one thread, the tables compared.
    python tools/dev_line_decode.py detect [--reps 40] [--line] [--margin] [--split] [--weight 16] [--ins 0] [--del 0] [--iters N]
        the detect call of tests/test_line_decode_pipeline.py (two 640 x 480 S-text frames, two pyramid levels, grouped stages, masks,
        frame lines, line words, run reading, word decode): every call time, median, minimum, maximum.  --line switches the setting on
        and prints the lines' strings beside the word gap's.  --margin (with --line) switches the margins on as well and prints every
        line's margin and its unsure breaks; without --iters it times the call with the margins off and on, alternated.  --split adds
        WANT_RUN_SPLIT: the rows are the words' parts and the line kernels run behind a second wait.
    python tools/dev_line_decode.py detect --lattice [--reps 40] [--weight 16] [--ins 0] [--del 0] [--iters N]
        the same call three ways, alternated: "second_wait" (WANT_WORD_DECODE and WANT_RUN_SPLIT with set_line_decode: the line decode
        on the split parts behind a wait of its own), "lattice" (WANT_RUN_SPLIT and WANT_LATTICE_DECODE) and "line_lattice" (the same
        with set_line_lattice_decode: k_line_lattice_decode behind k_lattice_decode, one wait); every call time, median, minimum,
        maximum, and the lines' strings.  --iters: calls of the first and the last only, for a trace with k_line_decode,
        k_lattice_decode and k_line_lattice_decode side by side.
"""
import argparse, gzip, json, os, sys, tempfile, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["kernel", "detect"])
ap.add_argument("--lines", type=int, default=100)
ap.add_argument("--rows", type=int, default=75)
ap.add_argument("--reps", type=int, default=0)
ap.add_argument("--iters", type=int, default=0)
ap.add_argument("--ins", type=int, default=0)
ap.add_argument("--del", dest="dele", type=int, default=0)
ap.add_argument("--weight", type=int, default=16)
ap.add_argument("--line", action="store_true")
ap.add_argument("--margin", action="store_true")
ap.add_argument("--split", action="store_true")
ap.add_argument("--lattice", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
    rng = np.random.default_rng(1)
    letters = np.array(list(ALPHABET))
    table = S.bigram_from_words(["".join(letters[rng.integers(0, 65, int(l))]) for l in rng.integers(3, 13, 2000)])
    n = a.lines * a.rows
    lfirst = (np.arange(a.lines) * a.rows).astype(np.int32)
    ln = np.full(a.lines, a.rows, np.int32)
    cuts = [0]
    while cuts[-1] < n:
        cuts.append(min(n, cuts[-1] + int(rng.integers(3, 13))))
    wfirst, wn = np.array(cuts[:-1], np.int32), np.diff(cuts).astype(np.int32)
    costs = rng.integers(40, 256, (n, 65))
    cheap = rng.random(costs.shape) < 0.05
    costs[cheap] = rng.integers(0, 16, int(cheap.sum()))
    costs = costs.astype(np.uint8)
    gaps = rng.integers(0, 64, (n, 2)).astype(np.uint8)
    f = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    f.set_bigram(table)
    f.set_word_decode(a.ins, a.dele)
    out = {"lib": S.lib_path(), "lines": a.lines, "rows_a_line": a.rows, "rows": n, "words": len(wn), "ins": a.ins, "del": a.dele}
    dec, chars, src, wor = f.decode_lines(costs, gaps, lfirst, ln)
    out["breaks"] = int(dec["n_breaks"].sum())
    out["table_bytes"] = f.line_decode_stats()["table_bytes"]
    if a.margin:
        mg = f.line_margins(costs, gaps, lfirst, ln)
        out["margin_table_bytes"] = f.line_margin_stats()["table_bytes"]
        out["gaps_with_an_alternative"] = int((mg[4] >= 0).sum())
        out["gap_margins_of_0"] = int((mg[4] == 0).sum())
    if a.lattice:          # the same lines over runs of 1 .. 4 atoms: the pieces' rows drawn as the runs' are
        splits = np.zeros(n, S.RUN_SPLIT_DTYPE)
        splits["n_cuts"] = rng.integers(0, 4, n)
        splits["cut"] = -1
        splits["n_pieces"] = np.array([0, 2, 5, 9])[splits["n_cuts"]]
        splits["first_piece"] = np.concatenate([[0], np.cumsum(splits["n_pieces"])[:-1]])
        pieces = rng.integers(40, 256, (int(splits["n_pieces"].sum()), 65))
        cheap = rng.random(pieces.shape) < 0.05
        pieces[cheap] = rng.integers(0, 16, int(cheap.sum()))
        pieces = pieces.astype(np.uint8)
        ll = f.lattice_decode_lines(splits, costs, pieces, gaps, lfirst, ln)
        out["lattice"] = {"nodes": int((splits["n_cuts"] + 1).sum()), "pieces": len(pieces), "parts": len(ll[3]), "breaks": int(ll[0]["n_breaks"].sum()),
                          "parts_that_are_pieces": int((ll[3]["piece"] >= 0).sum()), "table_bytes": f.line_lattice_decode_stats()["table_bytes"],
                          "cost_sum": int(ll[0]["cost"].sum()), "line_decode_cost_sum": int(dec["cost"].sum())}
    if a.iters:
        for _ in range(a.iters):
            f.decode_words(costs, wfirst, wn)
            f.decode_lines(costs, gaps, lfirst, ln)
            if a.lattice:
                f.lattice_decode_lines(splits, costs, pieces, gaps, lfirst, ln)
            if a.margin:
                f.line_margins(costs, gaps, lfirst, ln)
        out["iters"] = a.iters
    else:
        reps = a.reps or 7
        out["decode_lines_call_ms"] = timed(lambda: f.decode_lines(costs, gaps, lfirst, ln), reps)
        out["decode_words_call_ms"] = timed(lambda: f.decode_words(costs, wfirst, wn), reps)
        t0 = time.perf_counter()
        host = S.decode_lines_host(costs, gaps, lfirst, ln, table, a.ins, a.dele)
        dt = time.perf_counter() - t0
        assert all(x.tobytes() == y.tobytes() for x, y in zip(host, (dec, chars, src, wor)))
        out["host_one_thread_ms"] = round(dt * 1e3, 2)
        if a.lattice:
            out["lattice"]["lattice_decode_lines_call_ms"] = timed(lambda: f.lattice_decode_lines(splits, costs, pieces, gaps, lfirst, ln), reps)
            t0 = time.perf_counter()
            host = S.lattice_decode_lines_host(splits, costs, pieces, gaps, lfirst, ln, table, a.ins, a.dele)
            dt = time.perf_counter() - t0
            assert all(x.tobytes() == y.tobytes() for x, y in zip(host, ll))
            out["lattice"]["host_one_thread_ms"] = round(dt * 1e3, 2)
        if a.margin:
            out["line_margins_call_ms"] = timed(lambda: f.line_margins(costs, gaps, lfirst, ln), reps)
            t0 = time.perf_counter()
            host = S.line_margins_host(costs, gaps, lfirst, ln, table, a.ins, a.dele)
            dt = time.perf_counter() - t0
            assert all(x.tobytes() == y.tobytes() for x, y in zip(host, mg))
            out["margins_host_one_thread_ms"] = round(dt * 1e3, 2)
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
    out = {"lib": S.lib_path(), "line": a.line, "weight": a.weight, "ins": a.ins, "dele": a.dele, "lines": len(plain.texts), "runs": len(plain.line_runs),
           "words": len(plain.words), "longest_line_runs": int(plain.line_words["n_runs"].max(initial=0))}
    read = sorted({plain.word_text(w) for w in range(len(plain.words))})
    f.set_bigram(S.bigram_from_words([t for t in read if t and all(ch in ALPHABET for ch in t)]))
    f.set_word_decode(a.ins, a.dele)
    if a.lattice:
        return detect_lattice(f, frames, flags, out)
    flags |= S.WANT_WORD_DECODE | (S.WANT_RUN_SPLIT if a.split else 0)
    if a.line:
        f.set_line_decode(True, a.weight)
        r = f.text_detect(frames, flags)
        out["breaks"] = int(r.line_decodes["n_breaks"].sum())
        out["word_gap_breaks"] = int((r.line_words["n_words"].clip(1) - 1).sum())
        out["texts"] = [[r.line_decode_text(t), " ".join(r.words_decode_text_of_line(t))] for t in range(len(r.texts))]
        out["table_bytes"] = f.line_decode_stats()["table_bytes"]
    if a.line and a.margin:
        f.set_line_margin(True)
        r = f.text_detect(frames, flags)
        out["margins"] = [[r.line_decode_margin(t), [g for g in r.line_break_margins(t) if 0 <= g[2] < 8]] for t in range(len(r.texts))]
        out["margin_table_bytes"] = f.line_margin_stats()["table_bytes"]
    if a.iters:
        for _ in range(a.iters):
            f.text_detect(frames, flags)
        out["iters"] = a.iters
    elif a.line and a.margin:          # off and on, alternated
        off, on = [], []
        for k in range(5 + (a.reps or 40)):
            for t, flag in ((off, False), (on, True)):
                f.set_line_margin(flag)
                t0 = time.perf_counter()
                f.text_detect(frames, flags)
                if k >= 5:
                    t.append((time.perf_counter() - t0) * 1e3)
        out["detect_call_ms_margin_off"], out["detect_call_ms_margin_on"] = stats(off), stats(on)
    else:
        for _ in range(5):
            f.text_detect(frames, flags)
        out["detect_call_ms"] = timed(lambda: f.text_detect(frames, flags), a.reps or 40)
    f.close()
    return out


def detect_lattice(f, frames, flags, out):
    ways = {"second_wait": (flags | S.WANT_WORD_DECODE | S.WANT_RUN_SPLIT, True, False),
            "lattice": (flags | S.WANT_RUN_SPLIT | S.WANT_LATTICE_DECODE, False, False),
            "line_lattice": (flags | S.WANT_RUN_SPLIT | S.WANT_LATTICE_DECODE, False, True)}

    def call(way):
        fl, line, ll = ways[way]
        f.set_line_decode(line, a.weight)
        f.set_line_lattice_decode(ll, a.weight)
        return f.text_detect(frames, fl)

    r = call("line_lattice")
    out["pieces"] = len(r.run_pieces)
    out["nodes"] = int((r.run_splits["n_cuts"] + 1).sum())
    out["breaks"] = int(r.line_lattice_decodes["n_breaks"].sum())
    out["parts"] = len(r.line_lattice_parts)
    out["parts_that_are_pieces"] = int((r.line_lattice_parts["piece"] >= 0).sum())
    out["table_bytes"] = f.line_lattice_decode_stats()["table_bytes"]
    second = call("second_wait")
    out["texts"] = [[r.line_lattice_text(t), second.line_decode_text(t)] for t in range(len(r.texts))]
    if a.iters:
        for _ in range(a.iters):
            call("second_wait")
            call("line_lattice")
        out["iters"] = a.iters
    else:
        t = {w: [] for w in ways}
        for k in range(5 + (a.reps or 40)):
            for w in ways:
                t0 = time.perf_counter()
                call(w)
                if k >= 5:
                    t[w].append((time.perf_counter() - t0) * 1e3)
        out["detect_call_ms"] = {w: stats(v) for w, v in t.items()}
    f.close()
    return out


if __name__ == "__main__":
    res = kernel() if a.mode == "kernel" else detect()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
