"""A numpy reference of the joint decode over the piece lattice (str_er_lattice_decode in include/str_er.h), written from the
definition: the nodes and edges of a word's runs, the recurrence with the SPLIT penalty and the optional DEL and INS moves, the
backtrack with the lattice parts, and an enumeration of every path through the lattice with every string and every choice of moves
along it, for small alphabets.  The alphabet size is a parameter: the library's is 65, the boundary symbol is E = n.

A word is given as the cut counts of its runs, the first piece of every run and the two row tables (the runs', the pieces'); the
pieces of a run of A atoms are ordered by (i, j) over the nodes 0 .. A without (0, A), as str_er_run_split lists them."""
import itertools

import numpy as np

import word_decode_ref as WD

INF = 1 << 20
MAX_NODES = 32
LATTICE_FIELDS = ("cost", "read_cost", "n_chars", "n_sub", "n_del", "n_ins", "first_part", "n_parts")
SUB, DEL = 0, 1


def piece_of(A, i, j):
    """The index of the piece (i, j) in its run's list, -1 for the run itself."""
    if (i, j) == (0, A):
        return -1
    order = [(a, b) for a in range(A) for b in range(a + 1, A + 1) if (a, b) != (0, A)]
    return order.index((i, j))


def n_pieces(n_cuts):
    return (n_cuts + 1) * (n_cuts + 2) // 2 - 1 if n_cuts > 0 else 0


class Word:
    """The lattice of one word: rows[(r, i, j)] and part[(r, i, j)] = (run index in the table, piece index in the table or -1)."""

    def __init__(self, n_cuts, first_piece, run_rows, piece_rows, first_run=0, n=65):
        run_rows = np.asarray(run_rows, np.int64).reshape(-1, n)
        piece_rows = np.asarray(piece_rows, np.int64).reshape(-1, n)
        self.atoms = [int(k) + 1 for k in n_cuts]
        self.N = sum(self.atoms)
        self.off = [sum(self.atoms[:r]) for r in range(len(self.atoms))]
        self.rows, self.part = {}, {}
        for r, A in enumerate(self.atoms):
            for i in range(A):
                for j in range(i + 1, A + 1):
                    k = piece_of(A, i, j)
                    self.rows[r, i, j] = run_rows[first_run + r] if k < 0 else piece_rows[int(first_piece[r]) + k]
                    self.part[r, i, j] = (first_run + r, -1 if k < 0 else int(first_piece[r]) + k)
        self.own = run_rows[first_run:first_run + len(self.atoms)]


def decode_word(n_cuts, first_piece, run_rows, piece_rows, B, ins=0, dele=0, split=8, first_run=0, n=65):
    """One word: (record without first_part as a tuple: cost, read_cost, n_chars, n_sub, n_del, n_ins, n_parts; labels; sources; parts)."""
    L = Word(n_cuts, first_piece, run_rows, piece_rows, first_run, n)
    B = np.asarray(B, np.int64).reshape(n + 1, n + 1)
    E = n
    rc = WD.read_cost(L.own, B, n)
    if L.N > MAX_NODES:
        return (-1, rc, 0, 0, 0, 0, 0), [], [], []
    V = [np.full(n + 1, INF, np.int64)]
    V[0][E] = 0
    steps = [None]                                         # per node >= 1: (run, j, move, i, pred, is_ins, ins_pred)
    for r, A in enumerate(L.atoms):
        for j in range(1, A + 1):
            U = np.full(n + 1, INF, np.int64)
            move = np.zeros(n + 1, np.int64)
            frm = np.zeros(n + 1, np.int64)
            pred = np.zeros(n + 1, np.int64)
            for i in range(j):
                Vf = V[L.off[r] + i]
                s = split if i > 0 else 0
                cand = Vf[:, None] + B[:, :n]              # [a, b]
                S = cand.min(axis=0) + L.rows[r, i, j] + s
                a = cand.argmin(axis=0)                    # (numpy: the first of equal minima)
                better = S < U[:n]
                U[:n] = np.where(better, S, U[:n])
                move[:n] = np.where(better, SUB, move[:n]); frm[:n] = np.where(better, i, frm[:n]); pred[:n] = np.where(better, a, pred[:n])
                if dele > 0:
                    D = Vf + dele + s
                    better = D < U
                    U = np.where(better, D, U)
                    move = np.where(better, DEL, move); frm = np.where(better, i, frm)
            W = U.copy()
            is_ins = np.zeros(n + 1, bool)
            ins_pred = np.zeros(n + 1, np.int64)
            if ins > 0:
                ci = U[:n, None] + B[:n, :n]               # [b, c]
                I = ci.min(axis=0) + ins
                ins_pred[:n] = ci.argmin(axis=0)
                is_ins[:n] = I < U[:n]
                W[:n] = np.where(is_ins[:n], I, U[:n])
            V.append(W)
            steps.append((r, j, move, frm, pred, is_ins, ins_pred))
    end = V[L.N] + B[:, E]
    state = int(np.argmin(end))
    cost = int(end[state])
    assert cost < INF and max(int(v.max()) for v in V) < (1 << 21)     # (INF is never the minimum; every value is below 2^21)
    labels, src, parts = [], [], []
    n_sub = n_del = n_ins = 0
    node = L.N
    while node > 0:
        r, j, move, frm, pred, is_ins, ins_pred = steps[node]
        k = len(parts)                                     # (counted from the end until the number of parts is known)
        if is_ins[state]:
            labels.append(state); src.append((k, True)); n_ins += 1
            state = int(ins_pred[state])
        i = int(frm[state])
        parts.append(L.part[r, i, j])
        if move[state] == DEL:
            n_del += 1
        else:
            labels.append(state); src.append((k, False)); n_sub += 1
            state = int(pred[state])
        node = L.off[r] + i
    assert state == E
    labels.reverse(); src.reverse(); parts.reverse()
    src = [(len(parts) - 1 - k) | (0x80 if inserted else 0) for k, inserted in src]
    return (cost, rc, len(labels), n_sub, n_del, n_ins, len(parts)), labels, src, parts


def decode_words(splits, run_costs, piece_costs, first_run, n_of, B, ins=0, dele=0, split=8, n=65):
    """Every word of a call (splits: records with n_cuts and first_piece): the records as tuples in the order of LATTICE_FIELDS,
    chars and src (n_words, 64) uint8 padded with 0xFF, and the parts as an (n_parts, 2) int32 array."""
    recs, parts = [], []
    chars = np.full((len(first_run), 64), 0xFF, np.uint8)
    src = np.full((len(first_run), 64), 0xFF, np.uint8)
    for w, (f, k) in enumerate(zip(first_run, n_of)):
        f, k = int(f), int(k)
        cuts = [int(splits[r]["n_cuts"]) for r in range(f, f + k)]
        fps = [int(splits[r]["first_piece"]) for r in range(f, f + k)]
        rec, lab, s, pt = decode_word(cuts, fps, run_costs, piece_costs, B, ins, dele, split, f, n)
        recs.append(rec[:6] + (len(parts), rec[6]))
        parts += pt
        chars[w, :len(lab)] = lab
        src[w, :len(s)] = s
    return recs, chars, src, np.asarray(parts, np.int32).reshape(-1, 2)


def segmentations(A):
    """Every way through a run of A atoms: lists of edges (i, j) from node 0 to node A."""
    if A == 0:
        return [[]]
    return [[(0, j)] + [(i + j, k + j) for i, k in rest] for j in range(1, A + 1) for rest in segmentations(A - j)]


def enumerate_best(n_cuts, first_piece, run_rows, piece_rows, B, ins, dele, split, n):
    """The cheapest of every path through the lattice with every string and every choice of moves along it, by brute force: per edge one
    of DEL, SUB b, or either followed by one inserted character c (after some character).  A run's paths, strings and moves are all
    walked from every character the run before can end on -- the runs meet in that character alone -- and the minimum is kept per
    character."""
    L = Word(n_cuts, first_piece, run_rows, piece_rows, 0, n)
    B = np.asarray(B, np.int64).reshape(n + 1, n + 1)
    moves = ([("del",)] if dele > 0 else []) + [("sub", b) for b in range(n)]
    if ins > 0:
        moves += [("subins", b, c) for b in range(n) for c in range(n)]
        if dele > 0:
            moves += [("delins", c) for c in range(n)]
    best = {n: 0}
    for r, A in enumerate(L.atoms):
        nxt = {}
        for seg in segmentations(A):
            rows = [L.rows[r, i, j] for i, j in seg]
            pen = [split if i > 0 else 0 for i, j in seg]
            for path in itertools.product(moves, repeat=len(seg)):
                for start, c0 in best.items():
                    prev, s, ok = start, c0, True
                    for t, mv in enumerate(path):
                        s += pen[t]
                        if mv[0] == "del":
                            s += dele
                        elif mv[0] == "sub":
                            s += int(B[prev, mv[1]]) + int(rows[t][mv[1]]); prev = mv[1]
                        elif mv[0] == "subins":
                            s += int(B[prev, mv[1]]) + int(rows[t][mv[1]]) + int(B[mv[1], mv[2]]) + ins; prev = mv[2]
                        else:
                            if prev == n:                      # only after some character
                                ok = False
                                break
                            s += dele + int(B[prev, mv[1]]) + ins; prev = mv[1]
                    if ok and (prev not in nxt or s < nxt[prev]):
                        nxt[prev] = s
        best = nxt
    return min(c + int(B[prev, n]) for prev, c in best.items())


def path_cost(word, B, labels, src, parts, ins, dele, split, n=65):
    """The cost of a returned path and string under the definition: every part is read once or dropped, an inserted character pays INS,
    a part that does not begin its run pays SPLIT.  word: a Word; parts as (run, piece) of the tables."""
    B = np.asarray(B, np.int64).reshape(n + 1, n + 1)
    edge = {v: k for k, v in word.part.items()}
    keys = [edge[tuple(p)] for p in parts]
    s = sum(split for r, i, j in keys if i > 0)
    node = 0
    for r, i, j in keys:                                   # the parts are a path: each begins where the one before ended
        assert word.off[r] + i == node
        node = word.off[r] + j
    assert node == word.N
    prev, used = n, set()
    for a, t in zip(labels, src):
        s += int(B[prev, a])
        if t & 0x80:
            s += ins
        else:
            s += int(word.rows[keys[t]][a]); used.add(t)
        prev = a
    return s + int(B[prev, n]) + dele * (len(parts) - len(used))


def as_tuples(recs) -> list:
    """The library's LATTICE_DECODE_DTYPE records as tuples in the order of LATTICE_FIELDS."""
    return [tuple(int(r[k]) for k in LATTICE_FIELDS) for r in recs]
