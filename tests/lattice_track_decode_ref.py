"""A numpy reference of the track decode over the members' piece lattices (str_er_lattice_track_decode in include/str_er.h), written from
the contract alone on top of lattice_match_ref.py (the lattice, the recurrence vectorised over strings of one length, the backtrack with
the first-candidate rule), lattice_decode_ref.py (the seeds' strings) and track_decode_ref.py (lm and the neighbours of a string):
J(s) = lm(s) + the sum over the usable members of D_i[N_i][l], the seed with the smallest (J, rank), and the polish by single edits.
Every neighbour is scored with the full lattice recurrence -- there are no prefix or suffix tables here -- so it is independent of the
method of the kernel and of the host header.  It also returns the list of the edits it applied.

The words are given as for lattice_match_ref.match_words, the tracks as for track_decode_ref.decode_tracks."""
import numpy as np

import lattice_decode_ref as LD
import lattice_match_ref as LM
import track_decode_ref as TD

MAX_LEN, MAX_SEEDS = TD.MAX_LEN, TD.MAX_SEEDS
DECODE_FIELDS, NOT_DECODED = TD.DECODE_FIELDS, TD.NOT_DECODED
MEMBER_FIELDS = ("cost", "first_part", "n_parts", "n_del", "n_ins", "word")
SPLIT_DTYPE = np.dtype([("n_cuts", "<i4"), ("cut", "<i4", (3,)), ("thr", "<u4"), ("first_piece", "<i4"), ("n_pieces", "<i4"), ("n_parts", "<i4")])      # str_er_run_split


def word_lattice(splits, run_costs, piece_costs, first_run, n_of, w):
    f, k = int(first_run[w]), int(n_of[w])
    cuts = [int(splits[r]["n_cuts"]) for r in range(f, f + k)]
    fps = [int(splits[r]["first_piece"]) for r in range(f, f + k)]
    return LM.lattice(cuts, fps, run_costs, piece_costs, f, False)


def member_costs(L, strings, ins, dele, split) -> np.ndarray:
    """L(s) for every row of strings (n, l): the full recurrence over the lattice."""
    return LM.entry_costs(L, np.asarray(strings, np.int64), ins, dele, split)


def score(lats, s, B, ins, dele, split) -> int:
    return TD.lm(s, B) + sum(int(member_costs(L, [s], ins, dele, split)[0]) for L in lats)


def neighbour_scores(lats, s, B, ins, dele, split):
    """[(J, index, kind, j, a, string)] of every neighbour of s."""
    nb = TD.neighbours(s)
    B = np.asarray(B, np.int64).reshape(66, 66)
    J = np.zeros(len(nb), np.int64)
    for length in sorted({len(t[4]) for t in nb}):
        at = [i for i, t in enumerate(nb) if len(t[4]) == length]
        S = np.array([nb[i][4] for i in at], np.int64)
        J[at] = B[TD.E, S[:, 0]] + B[S[:, :-1], S[:, 1:]].sum(axis=1) + B[S[:, -1], TD.E]
        for L in lats:
            J[at] += member_costs(L, S, ins, dele, split)
    return [(int(J[i]),) + nb[i] for i in range(len(nb))]


def decode_track(splits, run_costs, piece_costs, first_run, n_of, members, B, dec_ins=0, dec_del=0, ins=64, dele=64, rounds=8, split=8):
    """One track: (record as a tuple in the order of DECODE_FIELDS; labels; per member (cost, n_parts, n_del, n_ins, word); per member its
    source bytes; per member its parts as (run, piece); the edits as [(kind, j, a)])."""
    lats = [word_lattice(splits, run_costs, piece_costs, first_run, n_of, int(w)) for w in members]
    usable = [i for i, L in enumerate(lats) if L.N <= LM.MAX_NODES]
    use = [lats[i] for i in usable]
    mrec = [(-1, 0, 0, 0, int(w)) for w in members]
    src, parts = [[] for _ in members], [[] for _ in members]
    seeds = []
    for i in usable:
        w = int(members[i])
        f, k = int(first_run[w]), int(n_of[w])
        _, lab, _, _ = LD.decode_word([int(splits[r]["n_cuts"]) for r in range(f, f + k)], [int(splits[r]["first_piece"]) for r in range(f, f + k)], run_costs,
                                      piece_costs, B, dec_ins, dec_del, split, f)
        if 1 <= len(lab) <= MAX_LEN and len(seeds) < MAX_SEEDS:
            seeds.append((i, [int(a) for a in lab]))
    if not seeds:
        return NOT_DECODED[:5] + (len(usable),) + NOT_DECODED[6:], [], mrec, src, parts, []
    J, rank = min((score(use, s, B, ins, dele, split), k) for k, (_, s) in enumerate(seeds))
    s = list(seeds[rank][1])
    seed_cost, seed_member = J, int(members[seeds[rank][0]])
    edits, converged = [], 0
    for _ in range(rounds):
        Jb, _, kind, j, a, t = min(neighbour_scores(use, s, B, ins, dele, split))
        if Jb < J:
            s, J = t, Jb
            edits.append((kind, j, a))
        else:
            converged = 1
            break
    for i in usable:
        cost, pt, sr, n_del, n_ins = LM.backtrack(lats[i], s, ins, dele, split)
        mrec[i] = (cost, len(pt), n_del, n_ins, int(members[i]))
        src[i], parts[i] = sr, [lats[i].part[k] for k in pt]
    return (J, seed_cost, len(s), len(edits), converged, len(usable), seed_member, TD.lm(s, B)), s, mrec, src, parts, edits


def decode_tracks(splits, run_costs, piece_costs, first_run, n_of, track_first, track_count, members, B, dec_ins=0, dec_del=0, ins=64, dele=64, rounds=8, split=8):
    """Every track of a call: the records as tuples (DECODE_FIELDS), chars (n_tracks, 32) uint8 padded with 0xFF, the member records as
    tuples (MEMBER_FIELDS) per slot of members, the sources (slots, 32) uint8 padded with 0xFF, the parts as an (n_parts, 2) int32 array in
    slot order, and the edits of every track."""
    nm = len(members)
    recs, edits = [], []
    chars = np.full((len(track_first), 32), 0xFF, np.uint8)
    rec, src_of, parts_of = [(-1, 0, 0, 0, -1)] * nm, [[] for _ in range(nm)], [[] for _ in range(nm)]
    for g, (f, n) in enumerate(zip(track_first, track_count)):
        f, n = int(f), int(n)
        r, s, mrec, src, parts, ed = decode_track(splits, run_costs, piece_costs, first_run, n_of, [int(w) for w in members[f:f + n]], B, dec_ins, dec_del, ins, dele,
                                                  rounds, split)
        recs.append(r)
        edits.append(ed)
        chars[g, :len(s)] = s
        rec[f:f + n], src_of[f:f + n], parts_of[f:f + n] = mrec, src, parts
    src = np.full((nm, 32), 0xFF, np.uint8)
    mrecs, all_parts = [], []
    for i in range(nm):
        mrecs.append((rec[i][0], len(all_parts)) + tuple(rec[i][1:]))
        all_parts += parts_of[i]
        src[i, :len(src_of[i])] = src_of[i]
    return recs, chars, mrecs, src, np.asarray(all_parts, np.int32).reshape(-1, 2), edits


as_tuples = TD.as_tuples


def members_as_tuples(mrec) -> list:
    """The library's LATTICE_TRACK_MEMBER_DTYPE records as tuples in the order of MEMBER_FIELDS."""
    return [tuple(int(r[k]) for k in MEMBER_FIELDS) for r in mrec]


def glyph_row(rng, a, confuse):
    """A plausible row of a glyph that reads a, as track_decode_ref.make_track makes it."""
    r = rng.integers(90, 256, 65)
    if rng.random() < confuse:
        r[int(rng.integers(0, 65))] = int(rng.integers(0, 30))      # another character reads best
        r[a] = int(rng.integers(20, 70))
    else:
        r[a] = int(rng.integers(0, 30))
    return r


def make_track(rng, truth, n_members, drop=0.15, add=0.15, confuse=0.25, touch=0.3):
    """The recipe of the tests, track_decode_ref.make_track extended with touching glyphs: n_members readings of the labels `truth`, each
    of which drops, adds and confuses runs, and with the probability `touch` merges two neighbouring truth characters into one run with
    1 .. 3 cuts.  The merged run reads badly as a whole; one of its cuts is the true one: the piece before it reads the first character,
    the piece behind it the second, and every other piece is noise.  Returns the members as a list of words, a word a list of runs
    (n_cuts, run row, piece rows in the order of str_er_run_split)."""
    out = []
    for _ in range(n_members):
        runs, t = [], 0
        while t < len(truth):
            if rng.random() < add:
                runs.append((0, rng.integers(60, 200, 65), []))      # a speck: nothing stands out
            if t + 1 < len(truth) and rng.random() < touch:
                k = int(rng.integers(1, 4))
                A, true_cut = k + 1, int(rng.integers(1, k + 1))      # the atoms before the true cut: 1 .. k
                pieces = []
                for i in range(A):
                    for j in range(i + 1, A + 1):
                        if (i, j) == (0, A):
                            continue
                        if (i, j) == (0, true_cut):
                            pieces.append(glyph_row(rng, truth[t], confuse))
                        elif (i, j) == (true_cut, A):
                            pieces.append(glyph_row(rng, truth[t + 1], confuse))
                        else:
                            pieces.append(rng.integers(110, 256, 65))
                runs.append((k, rng.integers(100, 256, 65), pieces))
                t += 2
                continue
            if rng.random() >= drop:
                runs.append((0, glyph_row(rng, truth[t], confuse), []))
            t += 1
        out.append(runs)
    return out


def pack(tracks):
    """Tracks as lists of words (make_track) -> (splits, run_costs, piece_costs, first_run, n_of, track_first, track_count, members): a
    word per member, in order."""
    words = [w for t in tracks for w in t]
    runs = [r for w in words for r in w]
    sp = np.zeros(len(runs), SPLIT_DTYPE)
    npc = [len(r[2]) for r in runs]
    sp["cut"] = -1
    sp["n_cuts"] = [r[0] for r in runs]
    sp["n_pieces"] = npc
    sp["first_piece"] = np.concatenate([[0], np.cumsum(npc)[:-1]]) if runs else []
    rr = np.array([r[1] for r in runs], np.uint8).reshape(-1, 65)
    pr = np.array([p for r in runs for p in r[2]], np.uint8).reshape(-1, 65)
    n_of = np.array([len(w) for w in words], np.int32)
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]]).astype(np.int32) if len(words) else np.zeros(0, np.int32)
    count = np.array([len(t) for t in tracks], np.int32)
    tfirst = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int32) if len(tracks) else np.zeros(0, np.int32)
    return sp, rr, pr, first, n_of, tfirst, count, np.arange(len(words), dtype=np.int32)
