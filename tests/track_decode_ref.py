"""A numpy reference of the track decode (str_er_track_decode in include/str_er.h), written from the contract alone on top of
word_match_ref.py (the recurrence) and word_decode_ref.py (the seeds' strings): J(s) = lm(s) + the sum over the usable members of
D[m][l], the set median of the seeds, and the polish by single edits.  Every neighbour is scored with the full recurrence -- there are
no prefix or suffix tables here -- so it is independent of the method of the kernel and of the host header.  It also returns the list of
the edits it applied."""
import numpy as np

import word_decode_ref as WD
import word_match_ref as WM

E = 65
MAX_LEN = 32
MAX_SEEDS = 32
MAX_MEMBERS = 1024
DEL_AT = 2080
INS_AT = 2112
DECODE_FIELDS = ("cost", "seed_cost", "n_chars", "n_edits", "converged", "n_used", "seed_member", "lm_cost")
NOT_DECODED = (-1, -1, 0, 0, 0, 0, -1, -1)


def lm(s, B) -> int:
    B = np.asarray(B, np.int64).reshape(66, 66)
    path = [E] + [int(a) for a in s] + [E]
    return sum(int(B[a, b]) for a, b in zip(path[:-1], path[1:]))


def align(C, strings, ins, dele) -> np.ndarray:
    """A(s) for every row of strings (n, l) on the rows C (m, 65): the full recurrence."""
    return WM.entry_costs(np.asarray(C, np.int64).reshape(-1, 65), np.asarray(strings, np.int64), ins, dele)


def score(rows, s, B, ins, dele) -> int:
    return lm(s, B) + sum(int(align(C, np.array([s]), ins, dele)[0]) for C in rows)


def neighbours(s):
    """[(index, kind, j, a, string)] of every neighbour of s that exists, ascending by index."""
    l, out = len(s), []
    for j in range(l):
        for a in range(65):
            out.append((j * 65 + a, "SUB", j, a, s[:j] + [a] + s[j + 1:]))
    if l > 1:
        for j in range(l):
            out.append((DEL_AT + j, "DEL", j, -1, s[:j] + s[j + 1:]))
    if l < MAX_LEN:
        for j in range(l + 1):
            for a in range(65):
                out.append((INS_AT + j * 65 + a, "INS", j, a, s[:j] + [a] + s[j:]))
    return out


def neighbour_scores(rows, s, B, ins, dele):
    """[(J, index, kind, j, a, string)] of every neighbour of s."""
    nb = neighbours(s)
    B = np.asarray(B, np.int64).reshape(66, 66)
    J = np.zeros(len(nb), np.int64)
    for length in sorted({len(t[4]) for t in nb}):
        at = [i for i, t in enumerate(nb) if len(t[4]) == length]
        S = np.array([nb[i][4] for i in at], np.int64)
        J[at] = B[E, S[:, 0]] + B[S[:, :-1], S[:, 1:]].sum(axis=1) + B[S[:, -1], E]          # lm of every string of this length
        for C in rows:
            J[at] += align(C, S, ins, dele)
    return [(int(J[i]),) + nb[i] for i in range(len(nb))]


def decode_track(costs, first_run, n_of, members, B, dec_ins=0, dec_del=0, ins=64, dele=64, rounds=8):
    """One track: (record as a tuple in the order of DECODE_FIELDS, labels, member_cost list, edits as [(kind, j, a)])."""
    costs = np.asarray(costs, np.uint8).reshape(-1, 65)
    all_rows = [costs[int(first_run[w]):int(first_run[w]) + int(n_of[w])] for w in members]
    usable = [i for i, C in enumerate(all_rows) if len(C) <= 32]
    rows = [all_rows[i] for i in usable]
    seeds = []
    for i in usable:
        _, lab, _ = WD.decode_word(all_rows[i], B, dec_ins, dec_del)
        if 1 <= len(lab) <= MAX_LEN and len(seeds) < MAX_SEEDS:
            seeds.append((i, [int(a) for a in lab]))
    if not seeds:
        return NOT_DECODED[:5] + (len(usable),) + NOT_DECODED[6:], [], [-1] * len(members), []
    J, rank = min((score(rows, s, B, ins, dele), k) for k, (_, s) in enumerate(seeds))
    s = list(seeds[rank][1])
    seed_cost, seed_member = J, int(members[seeds[rank][0]])
    edits, converged = [], 0
    for _ in range(rounds):
        Jb, _, kind, j, a, t = min(neighbour_scores(rows, s, B, ins, dele))
        if Jb < J:
            s, J = t, Jb
            edits.append((kind, j, a))
        else:
            converged = 1
            break
    member_cost = [-1] * len(members)
    for i in usable:
        member_cost[i] = int(align(all_rows[i], np.array([s]), ins, dele)[0])
    return (J, seed_cost, len(s), len(edits), converged, len(usable), seed_member, lm(s, B)), s, member_cost, edits


def decode_tracks(costs, first_run, n_of, track_first, track_count, members, B, dec_ins=0, dec_del=0, ins=64, dele=64, rounds=8):
    """(a tuple per track, chars (n_tracks, 32) uint8 padded with 0xFF, member_cost per slot of members: -1 in a slot of no track, the
    edits of every track)."""
    recs, edits = [], []
    chars = np.full((len(track_first), 32), 0xFF, np.uint8)
    mc = np.full(len(members), -1, np.int64)
    for g, (f, n) in enumerate(zip(track_first, track_count)):
        rec, s, own, ed = decode_track(costs, first_run, n_of, [int(w) for w in members[int(f):int(f) + int(n)]], B, dec_ins, dec_del, ins, dele, rounds)
        recs.append(rec)
        edits.append(ed)
        chars[g, :len(s)] = s
        mc[int(f):int(f) + int(n)] = own
    return recs, chars, mc, edits


def as_tuples(recs) -> list:
    """The library's TRACK_DECODE_DTYPE records as tuples in the order of DECODE_FIELDS."""
    return [tuple(int(r[k]) for k in DECODE_FIELDS) for r in recs]


def make_track(rng, truth, n_members, drop=0.15, add=0.15, confuse=0.25):
    """The recipe of the tests: n_members readings of the labels `truth`, each of which drops, adds and confuses runs.  Returns the
    members' rows as a list of (m, 65) uint8 arrays."""
    out = []
    for _ in range(n_members):
        rows = []
        for a in truth:
            if rng.random() < add:
                rows.append(rng.integers(60, 200, 65))                 # a speck: nothing stands out
            if rng.random() < drop:
                continue
            r = rng.integers(90, 256, 65)
            if rng.random() < confuse:
                r[int(rng.integers(0, 65))] = int(rng.integers(0, 30))  # another character reads best
                r[a] = int(rng.integers(20, 70))
            else:
                r[a] = int(rng.integers(0, 30))
            rows.append(r)
        out.append(np.array(rows, np.uint8).reshape(-1, 65))
    return out


def pack(tracks):
    """Tracks as lists of row arrays -> (costs, first_run, n_of, track_first, track_count, members): a word per member, in order."""
    rows = [C for t in tracks for C in t]
    n_of = np.array([len(C) for C in rows], np.int32)
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]]).astype(np.int32) if len(rows) else np.zeros(0, np.int32)
    costs = np.concatenate([C.reshape(-1, 65) for C in rows]).astype(np.uint8) if len(rows) else np.zeros((0, 65), np.uint8)
    count = np.array([len(t) for t in tracks], np.int32)
    tfirst = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int32) if len(tracks) else np.zeros(0, np.int32)
    return costs, first, n_of, tfirst, count, np.arange(len(rows), dtype=np.int32)
