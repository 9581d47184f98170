#!/usr/bin/env python3
"""Developer aid: what the track pool costs (profiles/track_pool.md).

    python tools/dev_track_pool.py batch [--same-length] [--lattice] [--iters N] [--reps 7]
        the shape of `dev_track_read.py kernel`: 1000 random words (3 .. 12 runs, band 2) in 125 tracks of 8 against 100 000 random
        entries.  One batch into an empty pool (clear, add, read) beside match_tracks (or lattice_match_tracks) on the same tracks,
        in the same process: the call times, the cells of the recurrence either computes, the pool's read-modify-write bytes, and the
        records compared.  --iters: calls only, for a `rocprofv3 --kernel-trace --stats` run.
    python tools/dev_track_pool.py stream [--lattice] [--batches 10]
        ten successive batches, each adding 8 members to the same 125 tracks: pool add + read per batch beside match_tracks on all
        members so far, which is what a caller without the pool runs.  The records are compared after every batch.
    python tools/dev_track_pool.py slots [--slots 125]
        join (pairs of slots) and read on a pool of --slots slots with 8 members each.
    python tools/dev_track_pool.py decode [--per-track 8] [--keep K] [--rounds 8] [--iters N] [--reps 7]
        the decode pool (profiles/decode_pool.md) on the shape of `dev_track_decode.py kernel`: 125 tracks of --per-track readings of
        one truth string each, fed as --per-track additions of one member per track into a DecodePool of --keep (default
        --per-track): the time of every addition (upload, k_word_decode, k_dpool_keep, wait), of a read of the 125 slots
        (k_dpool_plan, k_track_decode, k_dpool_records, copy back, wait) and beside them decode_tracks on all members, which is
        what a caller without the pool runs for every batch.  The records are compared.  --iters: one process of fill and read
        rounds only, for a `rocprofv3 --kernel-trace --stats` run.
    python tools/dev_track_pool.py lattice-decode [--touch 0.2] [--per-track 8] [--keep K] [--rounds 8] [--iters N] [--reps 7]
        the lattice decode pool (profiles/lattice_decode_pool.md) on the workloads of `dev_lattice_track_decode.py kernel`: 125 tracks
        of --per-track readings (--touch 0: no cut anywhere; --touch p: that share of the neighbouring glyphs touch), fed as
        --per-track additions of one member per track into a LatticeDecodePool of --keep: the time of every addition (upload,
        k_lattice_decode, k_ldpool_keep, wait), of a read of the 125 slots (k_dpool_plan, k_ldpool_tracks, k_lattice_track_decode,
        k_lattice_track_decode_members, k_ldpool_records, copy back, wait) and beside them lattice_decode_tracks on all members.  The
        records are compared.  --iters: one process of fill and read rounds only, for a `rocprofv3 --kernel-trace --stats` run.
"""
import argparse, json, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["batch", "stream", "slots", "decode", "lattice-decode"])
ap.add_argument("--words", type=int, default=1000)
ap.add_argument("--per-track", type=int, default=8)
ap.add_argument("--entries", type=int, default=100000)
ap.add_argument("--batches", type=int, default=10)
ap.add_argument("--slots", type=int, default=125)
ap.add_argument("--keep", type=int, default=0)
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--touch", type=float, default=0.2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=0)
ap.add_argument("--same-length", action="store_true")
ap.add_argument("--lattice", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (the HIP runtime PyTorch brings, loaded first)
import str_er_amd as S  # noqa: E402

ALPHABET = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz&()"
SEVEN = ["entry", "cost", "second_entry", "second_cost", "free_cost", "n_tried", "n_used"]


def stats(t):
    return {"calls": [round(x, 3) for x in t], "median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def timed(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return stats(t)


def make(rng, n_words, n_tracks, per_track):
    """Words with their rows (and, for --lattice, split records and piece rows), in tracks of per_track."""
    n_of = rng.integers(3, 13, n_words).astype(np.int32)
    if a.same_length:
        n_of[:n_tracks * per_track] = np.repeat(n_of[:n_tracks], per_track)
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]]).astype(np.int32)
    rows = lambda n: np.where(rng.random((n, 65)) < 0.05, rng.integers(0, 16, (n, 65)), rng.integers(40, 256, (n, 65))).astype(np.uint8)
    rc = rows(int(n_of.sum()))
    sp = np.zeros(len(rc), S.RUN_SPLIT_DTYPE)
    sp["cut"] = -1
    if a.lattice:          # a third of the runs with one cut: a run of two atoms has the pieces (0, 1) and (1, 2)
        sp["n_cuts"] = rng.random(len(rc)) < 1 / 3
        sp["n_pieces"] = 2 * sp["n_cuts"]
        sp["first_piece"] = np.concatenate([[0], np.cumsum(sp["n_pieces"])[:-1]])
    pc = rows(int(sp["n_pieces"].sum()))
    tf = (np.arange(n_tracks) * per_track).astype(np.int32)
    return dict(n_of=n_of, first=first, rc=rc, sp=sp, pc=pc, tf=tf, tc=np.full(n_tracks, per_track, np.int32), mem=np.arange(n_tracks * per_track, dtype=np.int32))


def context(rng):
    letters = np.array(list(ALPHABET))
    words = ["".join(letters[rng.integers(0, 65, int(l))]) for l in rng.integers(3, 13, a.entries)]
    f = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    f.set_lexicon(words)
    f.set_word_match(64, 64, 2)
    return f, np.bincount([len(w) for w in words], minlength=33)


def adders(f, pool, W):
    if a.lattice:
        return (lambda slots: pool.add_lattice(W["sp"], W["rc"], W["pc"], W["first"], W["n_of"], W["tf"], W["tc"], W["mem"], slots),
                lambda: f.lattice_match_tracks(W["sp"], W["rc"], W["pc"], W["first"], W["n_of"], W["tf"], W["tc"], W["mem"])[0])
    return (lambda slots: pool.add(W["rc"], W["first"], W["n_of"], W["tf"], W["tc"], W["mem"], slots),
            lambda: f.match_tracks(W["rc"], W["first"], W["n_of"], W["tf"], W["tc"], W["mem"])[0])


def same(pool_rec, track_rec):
    return all((pool_rec[k] == track_rec[k]).all() for k in SEVEN)


def batch():
    rng = np.random.default_rng(1)
    f, lens = context(rng)
    n_tracks = a.words // a.per_track
    W = make(rng, a.words, n_tracks, a.per_track)
    pool = S.TrackPool(f, n_tracks, lattice=a.lattice)
    slots = np.arange(n_tracks, dtype=np.int32)
    add, match = adders(f, pool, W)
    nodes = W["n_of"] + np.add.reduceat(W["sp"]["n_cuts"], W["first"]) if a.lattice else W["n_of"]          # (the rows of the column: runs, or atoms)
    out = {"lib": S.lib_path(), "tracks": n_tracks, "per_track": a.per_track, "entries": a.entries, "same_length": a.same_length, "lattice": a.lattice,
           "lexicon": f.lexicon_info(), "pool": pool.info()}
    cells_match = 0
    for g in range(n_tracks):
        ms, rs = nodes[g * a.per_track:(g + 1) * a.per_track], W["n_of"][g * a.per_track:(g + 1) * a.per_track]
        tried = [l for l in range(1, 33) if any(max(1, int(r) - 2) <= l <= min(32, int(m) + 2) for r, m in zip(rs, ms))]
        cells_match += sum(int(lens[l]) * int(m) * l for m in ms for l in tried)
    out["dp_cells_track_match"] = cells_match
    out["dp_cells_pool_add"] = int(sum(int(lens[l]) * l for l in range(1, 33)) * int(nodes[:n_tracks * a.per_track].sum()))
    out["pool_row_rmw_bytes"] = 2 * 4 * 64 * int(f.lexicon_info()["n"] // 64 + 32) * n_tracks          # (an upper bound: a load and a store of every padded entry and track)
    def one():
        pool.clear(slots); add(slots); return pool.read(slots)
    got, want = one(), match()
    out["records_equal"] = bool(same(got, want))
    if a.iters:
        for _ in range(a.iters):
            one(); match()
        out["iters"] = a.iters
    else:
        out["pool_clear_add_read_call_ms"] = timed(one, a.reps)
        out["match_tracks_call_ms"] = timed(match, a.reps)
    pool.close(); f.close()
    return out


def stream():
    rng = np.random.default_rng(2)
    f, lens = context(rng)
    n_tracks = a.words // a.per_track
    pool = S.TrackPool(f, n_tracks, lattice=a.lattice)
    slots = np.arange(n_tracks, dtype=np.int32)
    out = {"lib": S.lib_path(), "tracks": n_tracks, "per_batch": a.per_track, "batches": a.batches, "entries": a.entries, "lattice": a.lattice, "per_batch_ms": []}
    batches = [make(rng, a.words, n_tracks, a.per_track) for _ in range(a.batches)]
    for k in range(a.batches):
        # what a caller without the pool runs: the track match on all members so far (member j of batch b of track g, rows shifted behind the batches before)
        off_r = np.cumsum([0] + [len(B["rc"]) for B in batches[:k + 1]]); off_w = np.cumsum([0] + [len(B["n_of"]) for B in batches[:k + 1]])
        off_p = np.cumsum([0] + [len(B["pc"]) for B in batches[:k + 1]])
        sp = np.concatenate([B["sp"] for B in batches[:k + 1]])
        sp["first_piece"] += np.repeat(off_p[:-1], [len(B["sp"]) for B in batches[:k + 1]]).astype(np.int32)
        All = dict(rc=np.concatenate([B["rc"] for B in batches[:k + 1]]), pc=np.concatenate([B["pc"] for B in batches[:k + 1]]), sp=sp,
                   first=np.concatenate([B["first"] + off_r[b] for b, B in enumerate(batches[:k + 1])]).astype(np.int32),
                   n_of=np.concatenate([B["n_of"] for B in batches[:k + 1]]),
                   mem=np.concatenate([[off_w[b] + g * a.per_track + j for b in range(k + 1) for j in range(a.per_track)] for g in range(n_tracks)]).astype(np.int32),
                   tf=(np.arange(n_tracks) * a.per_track * (k + 1)).astype(np.int32), tc=np.full(n_tracks, a.per_track * (k + 1), np.int32))
        add, _ = adders(f, pool, batches[k])
        _, match = adders(f, pool, All)
        t0 = time.perf_counter(); add(slots); got = pool.read(slots); t1 = time.perf_counter(); want = match(); t2 = time.perf_counter()
        out["per_batch_ms"].append({"batch": k, "pool_add_read": round((t1 - t0) * 1e3, 3), "match_all_so_far": round((t2 - t1) * 1e3, 3), "equal": bool(same(got, want)),
                                    "members": int(got["n_members"][0])})
    pool.close(); f.close()
    return out


def slots_mode():
    rng = np.random.default_rng(3)
    f, lens = context(rng)
    n = a.slots
    W = make(rng, n * a.per_track, n, a.per_track)
    pool = S.TrackPool(f, n, lattice=False)
    every = np.arange(n, dtype=np.int32)
    pool.add(W["rc"], W["first"], W["n_of"], W["tf"], W["tc"], W["mem"], every)
    out = {"lib": S.lib_path(), "slots": n, "entries": a.entries, "pool": pool.info(), "read_call_ms": timed(lambda: pool.read(every), a.reps)}
    t = []
    for s in range(0, n - 1, 2):          # every pair once: the odd slot into the even one
        t0 = time.perf_counter(); pool.join(s, [s + 1]); t.append((time.perf_counter() - t0) * 1e3)
    out["join_call_ms"] = stats(t)
    out["read_after_joins_call_ms"] = timed(lambda: pool.read(every), a.reps)
    pool.close(); f.close()
    return out


def decode_mode():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import track_decode_ref as TD
    rng = np.random.default_rng(1)
    n_tracks, per, keep = a.words // a.per_track, a.per_track, a.keep or a.per_track
    tracks = [TD.make_track(rng, [int(x) for x in rng.integers(0, 65, int(rng.integers(3, 13)))], per) for _ in range(n_tracks)]
    costs, first, n_of, tfirst, tcount, members = TD.pack(tracks)
    B = rng.integers(0, 90, (66, 66)).astype(np.uint8)
    f = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    f.set_bigram(B)
    f.set_track_decode(64, 64, a.rounds)
    pool = S.DecodePool(f, n_tracks, keep)
    slots = np.arange(n_tracks, dtype=np.int32)
    # addition j: member j of every track, a track of one member each, with the rows of those words alone
    adds = []
    for j in range(per):
        ws = members[tfirst + j]
        rows = np.concatenate([costs[first[w]:first[w] + n_of[w]] for w in ws])
        n = n_of[ws].astype(np.int32)
        adds.append((rows, np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int32), n, np.arange(n_tracks, dtype=np.int32), np.ones(n_tracks, np.int32),
                     np.arange(n_tracks, dtype=np.int32)))
    def fill():
        t = []
        pool.clear(slots)
        for args in adds:
            t0 = time.perf_counter(); pool.add(*args, slots); t.append((time.perf_counter() - t0) * 1e3)
        return t
    one_call = lambda: f.decode_tracks(costs, first, n_of, tfirst, tcount, members)
    info = pool.info()
    out = {"lib": S.lib_path(), "tracks": n_tracks, "per_track": per, "keep": keep, "rounds": a.rounds, "words": int(len(first)), "rows": int(len(costs)),
           "rows_of_an_addition": [int(len(x[0])) for x in adds], "pool": info, "device_bytes_per_slot": round((info["device_bytes"]) / n_tracks, 1),
           "store_bytes_per_kept_member": 2184}
    fill()
    got, ch, mc = pool.read(slots)
    want, wch, wmc = one_call()
    same = [k for k in want.dtype.names if k != "seed_member"]
    out["records_equal"] = bool(keep >= per and all((got[k] == want[k]).all() for k in same) and (ch == wch).all() and (mc[:, :per].reshape(-1) == wmc).all())
    if a.iters:
        for _ in range(a.iters):
            fill(); pool.read(slots); one_call()
        out["iters"] = a.iters
    else:
        t = np.array([fill() for _ in range(a.reps)])          # (reps, per): the j-th addition finds j members pooled
        out["add_call_ms"] = [stats(t[:, j].tolist()) for j in range(per)]
        out["read_decode_call_ms"] = timed(lambda: pool.read(slots), a.reps)
        out["decode_tracks_call_ms"] = timed(one_call, a.reps)
    pool.close(); f.close()
    return out


def lattice_decode_mode():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import lattice_track_decode_ref as R
    import track_decode_ref as TD
    rng = np.random.default_rng(1)
    n_tracks, per, keep = a.words // a.per_track, a.per_track, a.keep or a.per_track
    truths = lambda: [int(x) for x in rng.integers(0, 65, int(rng.integers(3, 13)))]
    if a.touch > 0:
        packed = R.pack([R.make_track(rng, truths(), per, touch=a.touch) for _ in range(n_tracks)])
    else:          # the tracks of the `decode` mode, every run a word's run without a cut
        costs, first, n_of, tfirst, tcount, members = TD.pack([TD.make_track(rng, truths(), per) for _ in range(n_tracks)])
        sp = np.zeros(len(costs), S.RUN_SPLIT_DTYPE)
        sp["cut"] = -1
        packed = (sp, costs, np.zeros((0, 65), np.uint8), first, n_of, tfirst, tcount, members)
    sp, rr, pr, first, n_of, tfirst, tcount, members = packed
    B = rng.integers(0, 90, (66, 66)).astype(np.uint8)
    f = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    f.set_bigram(B)
    f.set_track_decode(64, 64, a.rounds)
    pool = S.LatticeDecodePool(f, n_tracks, keep)
    slots = np.arange(n_tracks, dtype=np.int32)
    # addition j: member j of every track, a track of one member each, with the runs and pieces of those words alone
    adds = []
    for j in range(per):
        ws = members[tfirst + j]
        runs = np.concatenate([np.arange(first[w], first[w] + n_of[w]) for w in ws]).astype(np.int64)
        s = sp[runs].copy()
        rows = [pr[int(q["first_piece"]):int(q["first_piece"]) + int(q["n_pieces"])] for q in s]
        s["first_piece"] = np.concatenate([[0], np.cumsum(s["n_pieces"])[:-1]])
        n = n_of[ws].astype(np.int32)
        adds.append((s, rr[runs], np.concatenate(rows + [np.zeros((0, 65), np.uint8)]), np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int32), n,
                     np.arange(n_tracks, dtype=np.int32), np.ones(n_tracks, np.int32), np.arange(n_tracks, dtype=np.int32)))
    def fill():
        t = []
        pool.clear(slots)
        for args in adds:
            t0 = time.perf_counter(); pool.add_lattice(*args, slots); t.append((time.perf_counter() - t0) * 1e3)
        return t
    one_call = lambda: f.lattice_decode_tracks(*packed)
    info = pool.info()
    out = {"lib": S.lib_path(), "tracks": n_tracks, "per_track": per, "keep": keep, "rounds": a.rounds, "touch": a.touch, "words": int(len(first)), "runs": int(len(rr)),
           "pieces": int(len(pr)), "cut_runs": int((sp["n_cuts"] > 0).sum()), "pool": info, "device_bytes_per_slot": round(info["device_bytes"] / n_tracks, 1),
           "store_bytes_per_kept_member": 9072}
    fill()
    got = pool.read_lattice(slots)
    want = one_call()
    same = [k for k in want[0].dtype.names if k != "seed_member"]
    out["records_equal"] = bool(keep >= per and all((got[0][k] == want[0][k]).all() for k in same) and (got[1] == want[1]).all() and
                                (got[2][:, :per].reshape(-1) == want[2]["cost"]).all() and (got[4][:, :per].reshape(-1, 32) == want[3]).all() and
                                len(got[5]) == len(want[4]))
    if a.iters:
        for _ in range(a.iters):
            fill(); pool.read_lattice(slots); one_call()
        out["iters"] = a.iters
    else:
        t = np.array([fill() for _ in range(a.reps)])          # (reps, per): the j-th addition finds j members pooled
        out["add_call_ms"] = [stats(t[:, j].tolist()) for j in range(per)]
        out["read_lattice_call_ms"] = timed(lambda: pool.read_lattice(slots), a.reps)
        out["read_call_ms"] = timed(lambda: pool.read(slots), a.reps)
        out["lattice_decode_tracks_call_ms"] = timed(one_call, a.reps)
    pool.close(); f.close()
    return out


if __name__ == "__main__":
    res = {"batch": batch, "stream": stream, "slots": slots_mode, "decode": decode_mode, "lattice-decode": lattice_decode_mode}[a.mode]()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
