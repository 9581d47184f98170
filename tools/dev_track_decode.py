#!/usr/bin/env python3
"""Developer aid: what the track decode and STR_ER_WANT_TRACK_DECODE cost (profiles/track_decode.md).

    python tools/dev_track_decode.py kernel [--words 1000] [--per-track 8] [--rounds 8] [--entries 100000] [--reps 7] [--iters N]
        decode_tracks on the shape of dev_track_read.py kernel: tracks of --per-track members, every track the readings of one truth
        string of 3 .. 12 labels whose members drop, add and confuse runs (the recipe of tests/track_decode_ref.py), under a random
        table: the time of every call (upload, k_word_decode, k_track_decode, copy back, wait), the rounds the tracks took, and beside
        it str_er_decode_tracks_host on one core and match_tracks of the same tracks against a random lexicon of --entries.  The
        records are compared with the host entry point.  --iters: calls only, for a `rocprofv3 --kernel-trace --stats` run, which
        gives the kernel times of k_track_decode and of k_track_match / _final side by side.
    python tools/dev_track_decode.py detect [--root DIR] [--reps 20] [--decode]
        the list call of tests/test_track_decode_pipeline.py (the 16-frame video, three pyramid levels, grouped stages, masks, frame
        lines, line links, line words, run reading, word decode): every call time, median, minimum, maximum.  --root runs another
        checkout (the parent), --decode adds the flag.
"""
import argparse, gzip, json, os, sys, tempfile, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["kernel", "detect"])
ap.add_argument("--words", type=int, default=1000)
ap.add_argument("--per-track", type=int, default=8)
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--entries", type=int, default=100000)
ap.add_argument("--reps", type=int, default=0)
ap.add_argument("--iters", type=int, default=0)
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


def timed(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return stats(t)


def kernel():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import track_decode_ref as TD
    rng = np.random.default_rng(1)
    n_tracks = a.words // a.per_track
    tracks = [TD.make_track(rng, [int(x) for x in rng.integers(0, 65, int(rng.integers(3, 13)))], a.per_track) for _ in range(n_tracks)]
    costs, first, n_of, tfirst, tcount, members = TD.pack(tracks)
    B = rng.integers(0, 90, (66, 66)).astype(np.uint8)
    f = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    f.set_bigram(B)
    f.set_track_decode(64, 64, a.rounds)
    out = {"lib": S.lib_path(), "words": int(len(first)), "rows": int(len(costs)), "tracks": n_tracks, "per_track": a.per_track, "rounds": a.rounds,
           "runs_of_a_member": {"min": int(n_of.min()), "median": float(np.median(n_of)), "max": int(n_of.max())}}
    decode = lambda: f.decode_tracks(costs, first, n_of, tfirst, tcount, members)
    got, ch, mc = decode()
    taken = got["n_edits"] + got["converged"]          # the rounds a track ran
    out["rounds_taken"] = {"mean": round(float(taken.mean()), 2), "max": int(taken.max()), "sum": int(taken.sum()), "histogram": np.bincount(taken).tolist()}
    out["edits"] = np.bincount(got["n_edits"]).tolist()
    out["converged"] = int(got["converged"].sum())
    out["string_lengths"] = {"min": int(got["n_chars"].min()), "median": float(np.median(got["n_chars"])), "max": int(got["n_chars"].max())}
    match = None
    if a.entries:
        letters = np.array(list(ALPHABET))
        f.set_lexicon(["".join(letters[rng.integers(0, 65, int(l))]) for l in rng.integers(3, 13, a.entries)])
        f.set_word_match(64, 64, 2)
        match = lambda: f.match_tracks(costs, first, n_of, tfirst, tcount, members)
        match()
        out["entries"] = a.entries
    if a.iters:
        for _ in range(a.iters):
            decode()
            if match:
                match()
        out["iters"] = a.iters
    else:
        out["decode_tracks_call_ms"] = timed(decode, a.reps or 7)
        out["decode_words_call_ms"] = timed(lambda: f.decode_words(costs, first, n_of), a.reps or 7)
        if match:
            out["match_tracks_call_ms"] = timed(match, a.reps or 7)
        t0 = time.perf_counter()
        host, hch, hmc = S.decode_tracks_host(costs, first, n_of, tfirst, tcount, members, B, 0, 0, 64, 64, a.rounds)
        dt = time.perf_counter() - t0
        assert host.tobytes() == got.tobytes() and hch.tobytes() == ch.tobytes() and hmc.tobytes() == mc.tobytes()
        out["host_one_thread_ms"] = round(dt * 1e3, 1)
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
    read = [t for t in sorted({plain.word_text(w) for w in range(len(plain.words))}) if 1 <= len(t) <= 32]
    f.set_bigram(S.bigram_from_words(read))
    flags |= S.WANT_WORD_DECODE
    out = {"root": os.path.abspath(a.root), "lib": S.lib_path(), "decode": a.decode, "lines": len(plain.texts), "runs": len(plain.line_runs), "words": len(plain.words)}
    if a.decode:
        flags |= S.WANT_TRACK_DECODE
        r = f.text_detect_list(frames, flags)
        d = r.track_decodes
        out.update(word_tracks=len(r.word_tracks), longest_track=int(r.word_tracks["count"].max()) if len(r.word_tracks) else 0, decoded=int((d["cost"] >= 0).sum()),
                   edits=np.bincount(d["n_edits"]).tolist(), converged=int(d["converged"].sum()))
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
