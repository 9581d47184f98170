"""A numpy reference of the lexicon match over the piece lattice (str_er_lattice_match in include/str_er.h), written from the
definition: the nodes and edges of a word's runs (lattice_decode_ref.Word), the recurrence over (node, character) with the SPLIT
penalty, vectorised over the entries of one length, the band of lengths, the best / second result of a word, the backtrack that takes
the first candidate in the contract's order, and the enumeration the contract names as equivalent: the minimum over all segmentations
of the word of the plain matcher's cost (word_match_ref) on the parts' rows plus SPLIT per part beyond the runs.

A word is given as the cut counts of its runs, the first piece of every run and the two row tables, as in lattice_decode_ref."""
import itertools

import numpy as np

import lattice_decode_ref as LD
import word_match_ref as WM

MAX_NODES = 32
MATCH_FIELDS = ("entry", "cost", "second_entry", "second_cost", "free_cost", "n_tried", "first_part", "n_parts", "n_del", "n_ins")


def lattice(n_cuts, first_piece, run_rows, piece_rows, first_run=0, fold=False):
    """The word's lattice with the rows as the matcher reads them: folded where the lexicon folds."""
    L = LD.Word(n_cuts, first_piece, run_rows, piece_rows, first_run)
    if fold:
        L.rows = {k: np.minimum(v, v[WM.PARTNER]) for k, v in L.rows.items()}
    L.node = [None]                                            # per node >= 1: (run, local index)
    for r, A in enumerate(L.atoms):
        L.node += [(r, j) for j in range(1, A + 1)]
    return L


def tables(L, E, ins, dele, split):
    """D[n][j] for every row of E (entries of one length, as labels): an (N + 1, l + 1, entries) array."""
    E = np.asarray(E, np.int64).reshape(len(E), -1)
    ne, l = E.shape
    D = np.zeros((L.N + 1, l + 1, ne), np.int64)
    D[0] = (np.arange(l + 1) * ins)[:, None]
    for n in range(1, L.N + 1):
        r, jl = L.node[n]
        for j in range(l + 1):
            cand = []
            for i in range(jl):
                f, s = L.off[r] + i, split if i > 0 else 0
                if j >= 1:
                    cand.append(D[f, j - 1] + L.rows[r, i, jl][E[:, j - 1]] + s)
                cand.append(D[f, j] + dele + s)
            if j >= 1:
                cand.append(D[n, j - 1] + ins)
            D[n, j] = np.min(cand, axis=0)
    return D


def entry_costs(L, E, ins, dele, split):
    return tables(L, E, ins, dele, split)[L.N, -1]


def in_band(R, N, l, band):
    return N <= MAX_NODES and max(1, R - band) <= l <= min(32, N + band)


def free_cost(L, split):
    """The str_er_word_split cost: every run's cheapest segmentation on the minima of its rows."""
    return sum(min(sum(int(L.rows[r, i, j].min()) + (split if i > 0 else 0) for i, j in seg) for seg in LD.segmentations(A)) for r, A in enumerate(L.atoms))


def backtrack(L, e, ins, dele, split):
    """(cost, parts as lattice keys (r, i, j) in word order, the source byte of every character, n_del, n_ins) of one entry."""
    D = tables(L, [e], ins, dele, split)[:, :, 0]
    n, j, parts, src, n_del, n_ins = L.N, len(e), [], [None] * len(e), 0, 0
    while n > 0 or j > 0:
        move = None
        if n > 0:
            r, jl = L.node[n]
            for i in range(jl):                                # the candidates in the contract's order: the first that attains the cell
                f, s = L.off[r] + i, split if i > 0 else 0
                if j >= 1 and D[f, j - 1] + L.rows[r, i, jl][e[j - 1]] + s == D[n, j]:
                    move = ("sub", i)
                    break
                if D[f, j] + dele + s == D[n, j]:
                    move = ("del", i)
                    break
        if move is None:
            assert j >= 1 and D[n, j - 1] + ins == D[n, j]
            src[j - 1] = ("ins", len(parts))                   # (the parts met so far all end behind the node n)
            n_ins += 1
            j -= 1
            continue
        i = move[1]
        if move[0] == "sub":
            src[j - 1] = ("sub", len(parts))
            j -= 1
        else:
            n_del += 1
        parts.append((r, i, jl))
        n = L.off[r] + i
    parts.reverse()
    np_ = len(parts)
    src = [0x80 | (np_ - k) if kind == "ins" else np_ - 1 - k for kind, k in src]
    return int(D[L.N, len(e)]), parts, src, n_del, n_ins


def match_word(n_cuts, first_piece, run_rows, piece_rows, lex: WM.Lexicon, ins=64, dele=64, band=2, split=8, first_run=0):
    """One word: (the record without first_part as a tuple: entry, cost, second_entry, second_cost, free_cost, n_tried, n_parts,
    n_del, n_ins; the sources; the parts as (run, piece) of the tables)."""
    L = lattice(n_cuts, first_piece, run_rows, piece_rows, first_run, lex.fold)
    R, free, keys = len(L.atoms), free_cost(L, split), []
    for l, (ix, E) in lex.by_len.items():
        if in_band(R, L.N, l, band):
            keys += list(zip(entry_costs(L, E, ins, dele, split).tolist(), ix.tolist()))
    keys.sort()
    best = keys[0] if keys else (-1, -1)
    second = keys[1] if len(keys) > 1 else (-1, -1)
    if not keys:
        return (-1, -1, -1, -1, free, 0, 0, 0, 0), [], []
    e = [WM.LABEL_OF[ch] for ch in lex.words[best[1]]]
    cost, parts, src, n_del, n_ins = backtrack(L, e, ins, dele, split)
    assert cost == best[0]
    return (best[1], best[0], second[1], second[0], free, len(keys), len(parts), n_del, n_ins), src, [L.part[k] for k in parts]


def match_words(splits, run_costs, piece_costs, first_run, n_of, lex, ins=64, dele=64, band=2, split=8):
    """Every word of a call (splits: records with n_cuts and first_piece): the records as tuples in the order of MATCH_FIELDS, the
    sources (n_words, 32) uint8 padded with 0xFF, and the parts as an (n_parts, 2) int32 array."""
    recs, parts = [], []
    src = np.full((len(first_run), 32), 0xFF, np.uint8)
    for w, (f, k) in enumerate(zip(first_run, n_of)):
        f, k = int(f), int(k)
        cuts = [int(splits[r]["n_cuts"]) for r in range(f, f + k)]
        fps = [int(splits[r]["first_piece"]) for r in range(f, f + k)]
        rec, s, pt = match_word(cuts, fps, run_costs, piece_costs, lex, ins, dele, band, split, f)
        recs.append(rec[:6] + (len(parts),) + rec[6:])
        parts += pt
        src[w, :len(s)] = s
    return recs, src, np.asarray(parts, np.int32).reshape(-1, 2)


def word_segmentations(L):
    """Every segmentation of the word: lists of lattice keys (r, i, j), one choice of LD.segmentations per run."""
    per_run = [[[(r, i, j) for i, j in seg] for seg in LD.segmentations(A)] for r, A in enumerate(L.atoms)]
    return [sum(choice, []) for choice in itertools.product(*per_run)]


def enumerate_costs(L, E, ins, dele, split):
    """cost(e) for every row of E by the contract's second form: the minimum over all segmentations P of the word of the
    str_er_word_match cost of e on the rows of P's parts (word_match_ref.entry_costs) + SPLIT * (|P| - n_runs).  L's rows are folded
    already where the lexicon folds."""
    E = np.asarray(E, np.int64).reshape(len(E), -1)
    best = None
    for P in word_segmentations(L):
        C = np.array([L.rows[k] for k in P], np.int64).reshape(len(P), 65)
        c = WM.entry_costs(C, E, ins, dele) + split * (len(P) - len(L.atoms))
        best = c if best is None else np.minimum(best, c)
    return best


def path_cost(L, e, src, parts, ins, dele, split):
    """The cost of a returned alignment under the definition: parts as lattice keys in word order; every part read once or dropped, an
    inserted character pays INS, a part that does not begin its run pays SPLIT.  Also checks that the parts are a path and that the
    sources are in order."""
    node = 0
    for r, i, j in parts:
        assert L.off[r] + i == node
        node = L.off[r] + j
    assert node == L.N
    s = sum(split for r, i, j in parts if i > 0)
    used, last = set(), -1
    for a, t in zip(e, src):
        if t & 0x80:
            assert last + 1 <= (t & 0x7F) <= len(parts)        # (inserted behind the parts read before it)
            s += ins
        else:
            assert t > last and t not in used
            s += int(L.rows[parts[t]][a])
            used.add(t)
            last = t
    return s + dele * (len(parts) - len(used))


def as_tuples(recs) -> list:
    """The library's LATTICE_MATCH_DTYPE records as tuples in the order of MATCH_FIELDS."""
    return [tuple(int(r[k]) for k in MATCH_FIELDS) for r in recs]
