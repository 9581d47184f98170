#!/usr/bin/env python3
"""Developer aid: what the track decode over the members' piece lattices and its setting cost (profiles/lattice_track_decode.md).

    python tools/dev_lattice_track_decode.py kernel [--words 1000] [--per-track 8] [--rounds 8] [--touch 0.2] [--reps 7] [--iters N]
        lattice_decode_tracks on the 125-tracks-of-8 shape of dev_track_decode.py kernel.  --touch 0: the very tracks of that tool,
        without a cut, with decode_tracks (the parent's k_track_decode) beside it on the same rows -- the outputs are compared byte for
        byte, so the ratio of the two kernels is the price of the lattice form alone.  --touch p > 0: the recipe of
        tests/lattice_track_decode_ref.py, two neighbouring characters merged into a run of 1 .. 3 cuts with the probability p.  The
        records are compared with the host entry point.  --iters: calls only, for a `rocprofv3 --kernel-trace --stats` run.
    python tools/dev_lattice_track_decode.py detect [--root DIR] [--reps 20] [--setting]
        the list call of tests/test_lattice_track_decode_pipeline.py (the 16-frame video, three pyramid levels, grouped stages, masks,
        frame lines, line links, line words, run reading, word decode, run split, track decode, lattice decode): every call time, median,
        minimum, maximum.  --root runs another checkout (the parent), --setting turns str_er_set_lattice_track_decode on.
"""
import argparse, gzip, json, os, sys, tempfile, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["kernel", "detect"])
ap.add_argument("--words", type=int, default=1000)
ap.add_argument("--per-track", type=int, default=8)
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--touch", type=float, default=0.2)
ap.add_argument("--reps", type=int, default=0)
ap.add_argument("--iters", type=int, default=0)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--setting", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import torch  # noqa: F401,E402  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S  # noqa: E402


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
    import lattice_track_decode_ref as R
    import track_decode_ref as TD
    rng = np.random.default_rng(1)
    n_tracks = a.words // a.per_track
    truths = lambda: [int(x) for x in rng.integers(0, 65, int(rng.integers(3, 13)))]
    plain = None
    if a.touch > 0:
        packed = R.pack([R.make_track(rng, truths(), a.per_track, touch=a.touch) for _ in range(n_tracks)])
    else:          # the tracks of dev_track_decode.py kernel, every run a word's run without a cut
        plain = TD.pack([TD.make_track(rng, truths(), a.per_track) for _ in range(n_tracks)])
        costs, first, n_of, tfirst, tcount, members = plain
        sp = np.zeros(len(costs), S.RUN_SPLIT_DTYPE)
        sp["cut"] = -1
        packed = (sp, costs, np.zeros((0, 65), np.uint8), first, n_of, tfirst, tcount, members)
    sp, rr, pr, first, n_of = packed[:5]
    B = rng.integers(0, 90, (66, 66)).astype(np.uint8)
    f = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    f.set_bigram(B)
    f.set_track_decode(64, 64, a.rounds)
    nodes = np.array([int((sp["n_cuts"][int(s):int(s) + int(n)] + 1).sum()) for s, n in zip(first, n_of)])
    edges = np.array([int(((sp["n_cuts"][int(s):int(s) + int(n)] + 1) * (sp["n_cuts"][int(s):int(s) + int(n)] + 2) // 2).sum()) for s, n in zip(first, n_of)])
    out = {"lib": S.lib_path(), "words": int(len(first)), "runs": int(len(rr)), "pieces": int(len(pr)), "cut_runs": int((sp["n_cuts"] > 0).sum()), "tracks": n_tracks,
           "per_track": a.per_track, "rounds": a.rounds, "touch": a.touch,
           "nodes_of_a_member": {"min": int(nodes.min()), "median": float(np.median(nodes)), "max": int(nodes.max())},
           "edges_of_a_member": {"min": int(edges.min()), "median": float(np.median(edges)), "max": int(edges.max())}}
    decode = lambda: f.lattice_decode_tracks(*packed)
    got = decode()
    taken = got[0]["n_edits"] + got[0]["converged"]          # the rounds a track ran
    out["rounds_taken"] = {"mean": round(float(taken.mean()), 2), "max": int(taken.max()), "sum": int(taken.sum()), "histogram": np.bincount(taken).tolist()}
    out["edits"] = np.bincount(got[0]["n_edits"]).tolist()
    out["converged"] = int(got[0]["converged"].sum())
    out["string_lengths"] = {"min": int(got[0]["n_chars"].min()), "median": float(np.median(got[0]["n_chars"])), "max": int(got[0]["n_chars"].max())}
    runs_decode = None
    if plain is not None:          # the parent's kernel on the same tracks: the same bytes
        runs_decode = lambda: f.decode_tracks(*plain)
        td, ch, mc = runs_decode()
        assert td.tobytes() == got[0].tobytes() and ch.tobytes() == got[1].tobytes() and mc.tolist() == got[2]["cost"].tolist()
        out["equals_decode_tracks"] = True
    if a.iters:
        for _ in range(a.iters):
            decode()
            if runs_decode:
                runs_decode()
        out["iters"] = a.iters
    else:
        out["lattice_decode_tracks_call_ms"] = timed(decode, a.reps or 7)
        if runs_decode:
            out["decode_tracks_call_ms"] = timed(runs_decode, a.reps or 7)
        t0 = time.perf_counter()
        host = S.lattice_decode_tracks_host(*packed, B, 0, 0, 64, 64, a.rounds, 8)
        dt = time.perf_counter() - t0
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, host))
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
    flags |= S.WANT_WORD_DECODE | S.WANT_RUN_SPLIT | S.WANT_TRACK_DECODE | S.WANT_LATTICE_DECODE
    out = {"root": os.path.abspath(a.root), "lib": S.lib_path(), "setting": a.setting, "lines": len(plain.texts), "runs": len(plain.line_runs), "words": len(plain.words)}
    if a.setting:
        f.set_lattice_track_decode(True)
        r = f.text_detect_list(frames, flags)
        d = r.lattice_track_decodes
        out.update(word_tracks=len(r.word_tracks), longest_track=int(r.word_tracks["count"].max()) if len(r.word_tracks) else 0, decoded=int((d["cost"] >= 0).sum()),
                   edits=np.bincount(d["n_edits"]).tolist(), converged=int(d["converged"].sum()), cut_runs=int((r.run_splits["n_cuts"] > 0).sum()),
                   strings_other_than_the_track_decodes=int((r.lattice_track_decode_chars != r.track_decode_chars).any(axis=1).sum()))
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
