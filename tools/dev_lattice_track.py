#!/usr/bin/env python3
"""Developer aid: what the track match over the members' piece lattices (STR_ER_WANT_LATTICE_TRACK, str_er_lattice_match_tracks) costs
(profiles/lattice_track.md).

    python tools/dev_lattice_track.py kernel [--words 1000] [--per-track 8] [--entries 100000] [--cuts] [--same-length] [--reps 7] [--iters N] [--what lattice|track|words]
        lattice_match_tracks on the words, rows and lexicon of tools/dev_track_read.py kernel (runs and entry lengths drawn from 3 .. 12,
        band 2, INS = DEL = 64, SPLIT = 8, fold) in tracks of --per-track: without --cuts every run is uncut and match_tracks on the same
        rows is timed in the same process (the yardstick: the same cells with --same-length); with --cuts every run has 0 .. 3 cuts and
        random piece rows, and lattice_match_words on the same words is the yardstick.  Prints every call time, the entries tried, the
        cells computed (member x entry tried x node x character x edges into the node), the table bytes, and the single-thread time of
        the host rules on the first tracks, with the records compared.  --iters: calls only (of --what: this entry point, match_tracks or
        lattice_match_words), for a `rocprofv3 --kernel-trace --stats` run, which gives the kernel times.  Runs on any checkout that has
        the entry point of --what (--root: the parent for `track` and `words`).
    python tools/dev_lattice_track.py detect [--root DIR] [--reps 40] [--flag]
        the detect call of tests/test_lattice_track_pipeline.py's shape (the two 640 x 480 S-text frames of the run-split pipeline test,
        each twice, two pyramid levels, grouped stages, masks, frame lines, line links, line words, run reading, run split, word match,
        track read, lattice match): every call time, median, minimum, maximum.  --root runs another checkout (the parent), --flag adds
        the lattice track match and prints how many tracks take another entry than the track match's.
"""
import argparse, gzip, json, os, sys, tempfile, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["kernel", "detect"])
ap.add_argument("--words", type=int, default=1000)
ap.add_argument("--per-track", type=int, default=8)
ap.add_argument("--entries", type=int, default=100000)
ap.add_argument("--cuts", action="store_true")
ap.add_argument("--same-length", action="store_true")
ap.add_argument("--host-tracks", type=int, default=3)
ap.add_argument("--reps", type=int, default=0)
ap.add_argument("--iters", type=int, default=0)
ap.add_argument("--what", choices=["lattice", "track", "words"], default="lattice")
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


def timed(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return stats(t)


def rows(rng, n):
    c = rng.integers(40, 256, (n, 65))
    cheap = rng.random(c.shape) < 0.05
    c[cheap] = rng.integers(0, 16, int(cheap.sum()))
    return c.astype(np.uint8)


def kernel():
    rng = np.random.default_rng(1)
    letters = np.array(list(ALPHABET))
    words = ["".join(letters[rng.integers(0, 65, int(l))]) for l in rng.integers(3, 13, a.entries)]
    n_tracks = a.words // a.per_track
    n_of = rng.integers(3, 13, a.words).astype(np.int32)
    if a.same_length:
        n_of[:n_tracks * a.per_track] = np.repeat(n_of[:n_tracks], a.per_track)
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]]).astype(np.int32)
    rc = rows(rng, int(n_of.sum()))                           # (the rows, words and lexicon of tools/dev_track_read.py kernel: the same draws)
    cuts = rng.integers(0, 4, len(rc)) if a.cuts else np.zeros(len(rc), np.int64)
    sp = np.zeros(len(rc), S.RUN_SPLIT_DTYPE)
    sp["cut"] = -1
    sp["n_cuts"] = cuts
    sp["n_pieces"] = np.where(cuts > 0, (cuts + 1) * (cuts + 2) // 2 - 1, 0)
    sp["first_piece"] = np.concatenate([[0], np.cumsum(sp["n_pieces"])[:-1]])
    pc = rows(rng, int(sp["n_pieces"].sum()))
    tfirst = (np.arange(n_tracks) * a.per_track).astype(np.int32)
    tcount = np.full(n_tracks, a.per_track, np.int32)
    members = np.arange(n_tracks * a.per_track, dtype=np.int32)
    f = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    f.set_lexicon(words)
    f.set_word_match(64, 64, 2)
    f.set_run_split(1, 4, 8)
    calls = {"lattice": lambda: f.lattice_match_tracks(sp, rc, pc, first, n_of, tfirst, tcount, members),
             "track": lambda: f.match_tracks(rc, first, n_of, tfirst, tcount, members),
             "words": lambda: f.lattice_match_words(sp, rc, pc, first, n_of)}
    out = {"lib": S.lib_path(), "words": a.words, "tracks": n_tracks, "per_track": a.per_track, "entries": a.entries, "cuts": a.cuts, "same_length": a.same_length,
           "lexicon": f.lexicon_info()}
    atoms = np.array([int((cuts[s:s + k] + 1).sum()) for s, k in zip(first, n_of)])
    edges = np.array([int(sum((c + 1) * (c + 2) // 2 for c in cuts[s:s + k])) for s, k in zip(first, n_of)])
    lens = np.bincount([len(w) for w in words], minlength=33)
    cells = cells_words = 0                                    # member x entry tried x node x character x edges into the node
    for g in range(n_tracks):
        ws = members[tfirst[g]:tfirst[g] + tcount[g]]
        tried = set()
        for w in ws:
            if atoms[w] <= 32:
                own = range(max(1, int(n_of[w]) - 2), min(32, int(atoms[w]) + 2) + 1)
                tried |= set(own)
                cells_words += sum(int(lens[l]) * int(edges[w]) * l for l in own)
        for w in ws:
            if atoms[w] <= 32:
                cells += sum(int(lens[l]) * int(edges[w]) * l for l in tried)
    out["dp_cells_tracks"], out["dp_cells_words"] = cells, cells_words
    if a.iters:
        for _ in range(a.iters):
            calls[a.what]()
        out["iters"], out["what"] = a.iters, a.what
    else:
        got = calls["lattice"]()
        out["tried"] = int(got[0]["n_tried"].astype(np.int64).sum())
        out["members_with_more_parts_than_runs"] = int((got[1]["n_parts"] > n_of[members]).sum())
        if not a.cuts:
            plain, mc = calls["track"]()
            assert got[0].tobytes() == plain.tobytes() and got[1]["cost"].tolist() == mc.tolist()
        tl, tm = [], []
        other = "words" if a.cuts else "track"
        for _ in range(a.reps or 7):                           # alternated in one process
            tl += timed(calls["lattice"], 1)["calls"]
            tm += timed(calls[other], 1)["calls"]
        out["lattice_match_tracks_call_ms"] = stats(tl)
        out[("lattice_match_words" if a.cuts else "match_tracks") + "_call_ms"] = stats(tm)
        nt = min(a.host_tracks, n_tracks)
        t0 = time.perf_counter()
        host = S.lattice_match_tracks_host(sp, rc, pc, first, n_of, tfirst[:nt], tcount[:nt], members[:nt * a.per_track], words, True, 64, 64, 2, 8)
        dt = time.perf_counter() - t0
        nm = nt * a.per_track
        n_parts = int(host[1]["n_parts"].sum())
        assert host[0].tobytes() == got[0][:nt].tobytes() and host[1].tobytes() == got[1][:nm].tobytes() and host[2].tobytes() == got[2][:nm].tobytes()
        assert host[3].tobytes() == got[3][:n_parts].tobytes()
        out["host_one_thread"] = {"tracks": nt, "ms": round(dt * 1e3, 1)}
        out["table_bytes"] = f.lattice_track_stats()
    f.close()
    return out


def detect():
    tmp = tempfile.mkdtemp(); sp, wp = S.cascade_io.write_golden(tmp)
    model = os.path.join(tmp, "ocr.model")
    with open(model, "wb") as fh:
        fh.write(gzip.open(S.cascade_io.ocr_model_path(5)).read())
    sy = S.synth
    two = [sy.stext_bgr(sy.frame_seed(2), 640, 480), sy.stext_bgr(sy.frame_seed(976), 640, 480)]
    frames = np.stack([two[0], two[0], two[1], two[1]])
    f = S.ERFilter(params=S.Params(max_width=640, max_height=480, max_frames=4, n_pyr_levels=2))
    f.load_cascade(0, sp); f.load_cascade(1, wp)
    f.load_svm_model(model, 1800)
    flags = S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP | S.WANT_MASKS | S.WANT_FRAME_LINES | S.WANT_LINE_LINKS | S.WANT_LINE_WORDS | S.WANT_RUN_READ | S.WANT_RUN_SPLIT
    plain = f.text_detect(frames, flags)
    rng = np.random.default_rng(9)
    read = sorted({plain.word_text(w) for w in range(len(plain.words))} | {plain.word_split_text(w) for w in range(len(plain.words))})
    read = [t for t in read if 1 <= len(t) <= 32]
    lexicon = read + ["".join(rng.choice(list(ALPHABET), int(rng.integers(1, 13)))) for _ in range(300)]
    f.set_lexicon(lexicon)
    flags |= S.WANT_WORD_MATCH | S.WANT_TRACK_READ | S.WANT_LATTICE_MATCH
    out = {"root": os.path.abspath(a.root), "lib": S.lib_path(), "flag": a.flag, "lines": len(plain.texts), "runs": len(plain.line_runs), "words": len(plain.words),
           "runs_with_a_cut": int((plain.run_splits["n_cuts"] > 0).sum()), "lexicon": len(lexicon)}
    if a.flag:
        flags |= S.WANT_LATTICE_TRACK
        r = f.text_detect(frames, flags)
        d, m, mem = r.lattice_track_matches, r.track_matches, r.lattice_track_members
        out.update(word_tracks=len(d), members=len(mem), longest_track=int(r.word_tracks["count"].max()) if len(d) else 0,
                   tracks_with_another_entry_than_the_track_match=int((d["entry"] != m["entry"]).sum()),
                   members_with_more_parts_than_runs=int((mem["n_parts"] > r.words["n_runs"][r.word_track_members]).sum()),
                   entries_tried=int(d["n_tried"].sum()), entries_tried_by_the_track_match=int(m["n_tried"].sum()), table_bytes=f.lattice_track_stats())
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
