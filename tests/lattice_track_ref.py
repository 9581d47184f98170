"""A numpy reference of the track match over the members' piece lattices (str_er_lattice_track_member in include/str_er.h), written from
the definition on top of lattice_match_ref (the lattice of a word, its tables vectorised over the entries of one length, the backtrack
with the first-candidate rule, the free cost) and track_read_ref (the order of a track record's fields): the usable members, the union
of their lattice bands, the sum of the members' costs per entry, the best / second result of a track, and for the winning entry every
member's own cost, parts and sources.

The words are given as for lattice_match_ref.match_words, the tracks as for track_read_ref.match_tracks."""
import numpy as np

import lattice_match_ref as LM
import track_read_ref as TR
import word_match_ref as WM

MEMBER_FIELDS = ("cost", "first_part", "n_parts", "n_del", "n_ins", "word")


def word_lattice(splits, run_costs, piece_costs, first_run, n_of, w, fold):
    f, k = int(first_run[w]), int(n_of[w])
    cuts = [int(splits[r]["n_cuts"]) for r in range(f, f + k)]
    fps = [int(splits[r]["first_piece"]) for r in range(f, f + k)]
    return LM.lattice(cuts, fps, run_costs, piece_costs, f, fold)


def match_track(splits, run_costs, piece_costs, first_run, n_of, members, lex: WM.Lexicon, ins=64, dele=64, band=2, split=8):
    """One track: (the str_er_track_match as a tuple in the order of track_read_ref.TRACK_FIELDS; per member (cost, n_parts, n_del,
    n_ins, word); per member its source bytes; per member its parts as (run, piece))."""
    lats = [word_lattice(splits, run_costs, piece_costs, first_run, n_of, int(w), lex.fold) for w in members]
    free = sum(LM.free_cost(L, split) for L in lats)
    usable = [i for i, L in enumerate(lats) if L.N <= LM.MAX_NODES]
    keys, own = [], {}
    for l, (ix, E) in lex.by_len.items():
        if not any(LM.in_band(len(lats[i].atoms), lats[i].N, l, band) for i in usable):
            continue
        per = np.array([LM.entry_costs(lats[i], E, ins, dele, split) for i in usable], np.int64).reshape(len(usable), len(ix))
        for col, e in enumerate(ix.tolist()):
            keys.append((int(per[:, col].sum()), e))
            own[e] = per[:, col].tolist()
    keys.sort()
    best = keys[0] if keys else (-1, -1)
    second = keys[1] if len(keys) > 1 else (-1, -1)
    mrec = [(-1, 0, 0, 0, int(w)) for w in members]
    src, parts = [[] for _ in members], [[] for _ in members]
    if keys:
        e = [WM.LABEL_OF[ch] for ch in lex.words[best[1]]]
        for i, c in zip(usable, own[best[1]]):
            cost, pt, s, n_del, n_ins = LM.backtrack(lats[i], e, ins, dele, split)
            assert cost == c
            mrec[i] = (cost, len(pt), n_del, n_ins, int(members[i]))
            src[i], parts[i] = s, [lats[i].part[k] for k in pt]
    have = [i for i in range(len(members)) if mrec[i][0] >= 0]
    best_member = int(members[min(have, key=lambda i: (mrec[i][0], i))]) if have else -1
    return (best[1], best[0], second[1], second[0], free, len(keys), len(usable), best_member), mrec, src, parts


def match_tracks(splits, run_costs, piece_costs, first_run, n_of, track_first, track_count, members, lex, ins=64, dele=64, band=2, split=8):
    """Every track of a call: the track records as tuples (TRACK_FIELDS), the member records as tuples (MEMBER_FIELDS) per slot of members,
    the sources (slots, 32) uint8 padded with 0xFF, and the parts as an (n_parts, 2) int32 array in slot order."""
    nm = len(members)
    out, rec, src_of, parts_of = [], [(-1, 0, 0, 0, -1)] * nm, [[] for _ in range(nm)], [[] for _ in range(nm)]
    for f, n in zip(track_first, track_count):
        f, n = int(f), int(n)
        r, mrec, src, parts = match_track(splits, run_costs, piece_costs, first_run, n_of, [int(w) for w in members[f:f + n]], lex, ins, dele, band, split)
        out.append(r)
        rec[f:f + n], src_of[f:f + n], parts_of[f:f + n] = mrec, src, parts
    src = np.full((nm, 32), 0xFF, np.uint8)
    mrecs, all_parts = [], []
    for i in range(nm):
        mrecs.append((rec[i][0], len(all_parts)) + tuple(rec[i][1:]))
        all_parts += parts_of[i]
        src[i, :len(src_of[i])] = src_of[i]
    return out, mrecs, src, np.asarray(all_parts, np.int32).reshape(-1, 2)


def members_as_tuples(mrec) -> list:
    """The library's LATTICE_TRACK_MEMBER_DTYPE records as tuples in the order of MEMBER_FIELDS."""
    return [tuple(int(r[k]) for k in MEMBER_FIELDS) for r in mrec]


as_tuples = TR.as_tuples
