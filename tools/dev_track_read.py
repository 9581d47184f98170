#!/usr/bin/env python3
"""Developer aid: what the track match and STR_ER_WANT_TRACK_READ cost (profiles/track_read.md).

    python tools/dev_track_read.py kernel [--words 1000] [--per-track 8] [--entries 100000] [--reps 7] [--iters N] [--same-length]
        match_tracks on random words (m and l drawn from 3 .. 12, band 2) in tracks of --per-track against a random lexicon, and
        match_words on the same words in the same process: the time of every call (upload, kernels, copy back, wait), and the cells
        of the recurrence either computes.  --same-length: the members of a track have one run count, as the readings of one word
        in several frames mostly do; then both compute the same cells.  The tracks' records are compared with the host rules on the
        first tracks.  --iters: calls only, for a `rocprofv3 --kernel-trace --stats` run, which gives the kernel times of
        k_track_match / _final and of k_word_match / _final side by side.
    python tools/dev_track_read.py detect [--root DIR] [--reps 20] [--track]
        the list call of tests/test_track_read_pipeline.py (the 16-frame video, three pyramid levels, grouped stages, masks, frame
        lines, line links, line words, run reading, word match): every call time, median, minimum, maximum.  --root runs another
        checkout (the parent), --track adds the flag and prints the stage's own lines of STR_ER_DEBUG_STATS where it is set.
"""
import argparse, gzip, json, os, sys, tempfile, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["kernel", "detect"])
ap.add_argument("--words", type=int, default=1000)
ap.add_argument("--per-track", type=int, default=8)
ap.add_argument("--entries", type=int, default=100000)
ap.add_argument("--reps", type=int, default=0)
ap.add_argument("--iters", type=int, default=0)
ap.add_argument("--same-length", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--track", action="store_true")
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
    rng = np.random.default_rng(1)
    letters = np.array(list(ALPHABET))
    words = ["".join(letters[rng.integers(0, 65, int(l))]) for l in rng.integers(3, 13, a.entries)]
    n_tracks = a.words // a.per_track
    n_of = rng.integers(3, 13, a.words).astype(np.int32)
    if a.same_length:
        n_of[:n_tracks * a.per_track] = np.repeat(n_of[:n_tracks], a.per_track)
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]]).astype(np.int32)
    costs = rng.integers(40, 256, (int(n_of.sum()), 65))
    cheap = rng.random(costs.shape) < 0.05
    costs[cheap] = rng.integers(0, 16, int(cheap.sum()))
    costs = costs.astype(np.uint8)
    tfirst = (np.arange(n_tracks) * a.per_track).astype(np.int32)
    tcount = np.full(n_tracks, a.per_track, np.int32)
    members = np.arange(n_tracks * a.per_track, dtype=np.int32)
    f = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    f.set_lexicon(words)
    f.set_word_match(64, 64, 2)
    out = {"lib": S.lib_path(), "words": a.words, "tracks": n_tracks, "per_track": a.per_track, "entries": a.entries, "lexicon": f.lexicon_info(),
           "same_length": a.same_length}
    track = lambda: f.match_tracks(costs, first, n_of, tfirst, tcount, members)
    word = lambda: f.match_words(costs, first, n_of)
    got, mc = track()
    word()
    lens = np.bincount([len(w) for w in words], minlength=33)
    out["dp_cells_words"] = int(sum(int(lens[l]) * int(m) * l for m in n_of for l in range(max(1, m - 2), min(32, m + 2) + 1)))
    cells = 0
    for g in range(n_tracks):
        ms = n_of[g * a.per_track:(g + 1) * a.per_track]
        tried = [l for l in range(1, 33) if any(abs(l - int(m)) <= 2 for m in ms)]
        cells += sum(int(lens[l]) * int(m) * l for m in ms for l in tried)
    out["dp_cells_tracks"] = cells
    if a.iters:
        for _ in range(a.iters):
            track()
            word()
        out["iters"] = a.iters
    else:
        out["match_tracks_call_ms"] = timed(track, a.reps or 7)
        out["match_words_call_ms"] = timed(word, a.reps or 7)
        nt = min(3, n_tracks)
        t0 = time.perf_counter()
        host, hmc = S.match_tracks_host(costs, first, n_of, tfirst[:nt], tcount[:nt], members[:nt * a.per_track], words, True, 64, 64, 2)
        dt = time.perf_counter() - t0
        assert host.tobytes() == got[:nt].tobytes() and hmc.tobytes() == mc[:nt * a.per_track].tobytes()
        out["host_one_thread"] = {"tracks": nt, "ms": round(dt * 1e3, 1)}
    f.close()
    return out


def detect():
    sys.path.insert(0, os.path.join(os.path.abspath(a.root), "tests"))
    from test_line_links import make_video
    tmp = tempfile.mkdtemp(); sp, wp = S.cascade_io.write_golden(tmp)
    model = os.path.join(tmp, "ocr.model")
    with open(model, "wb") as fh:
        fh.write(gzip.open(S.cascade_io.ocr_model_path(5)).read())
    frames, _ = make_video(S)
    f = S.ERFilter(params=S.Params(max_width=640, max_height=480, max_frames=16, n_pyr_levels=3))
    f.load_cascade(0, sp); f.load_cascade(1, wp)
    f.load_svm_model(model, 1800)
    flags = S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP | S.WANT_MASKS | S.WANT_FRAME_LINES | S.WANT_LINE_LINKS | S.WANT_LINE_WORDS | S.WANT_RUN_READ
    plain = f.text_detect_list(frames, flags)
    rng = np.random.default_rng(9)
    read = sorted({plain.word_text(w) for w in range(len(plain.words))})
    read = [t for t in read if 1 <= len(t) <= 32]
    lexicon = read + ["".join(rng.choice(list(ALPHABET), int(rng.integers(1, 13)))) for _ in range(300)]
    f.set_lexicon(lexicon)
    flags |= S.WANT_WORD_MATCH
    out = {"root": os.path.abspath(a.root), "lib": S.lib_path(), "track": a.track, "lines": len(plain.texts), "runs": len(plain.line_runs), "words": len(plain.words),
           "lexicon": len(lexicon)}
    if a.track:
        flags |= S.WANT_TRACK_READ
        r = f.text_detect_list(frames, flags)
        own = r.word_matches["entry"]
        differ = sum(any(int(own[w]) != int(m["entry"]) for w in r.word_track_members[int(t["first"]):int(t["first"]) + int(t["count"])])
                     for t, m in zip(r.word_tracks, r.track_matches))
        out.update(word_links=len(r.word_links), word_tracks=len(r.word_tracks), eligible_words=int((r.word_track_of_words >= 0).sum()),
                   longest_track=int(r.word_tracks["count"].max()) if len(r.word_tracks) else 0, tracks_whose_entry_differs_from_a_members_own=int(differ))
    for _ in range(3):
        f.text_detect_list(frames, flags)
    out["detect_call_ms"] = timed(lambda: f.text_detect_list(frames, flags), a.reps or 20)
    f.close()
    return out


if __name__ == "__main__":
    res = kernel() if a.mode == "kernel" else detect()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
