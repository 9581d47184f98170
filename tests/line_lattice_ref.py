"""A numpy reference of the joint decode of a text line over the piece lattices of its runs (str_er_line_lattice_decode in
include/str_er.h), written from the definition: the nodes of a line's runs, the gap step between two runs, the node step over the
edges of a run with the SPLIT penalty and the optional DEL and INS moves, the backtrack with the blanks, the parts and their words,
and an enumeration of every segmentation, every join / break choice, every string and every choice of moves, for small alphabets.
The alphabet size is a parameter: the library's is 65, the boundary symbol and the blank's label are E = n.

A line is given as lattice_decode_ref.Word gives a word -- the cut counts of its runs, the first piece of every run, the two row
tables -- with one gap pair (J, K) per run of the table, 255 meaning off; the pair of the line's first run is ignored."""
import itertools

import numpy as np

import lattice_decode_ref as LR

INF = 1 << 20
MAX_RUNS = 1024
OFF = 255
SRC_INS, SRC_BREAK = 0x8000, 0x4000
FIELDS = ("cost", "n_chars", "n_breaks", "n_sub", "n_del", "n_ins", "first_part", "n_parts")
SUB, DEL = 0, 1


def decode_line(n_cuts, first_piece, run_rows, piece_rows, gaps, B, ins=0, dele=0, split=8, first_run=0, n=65, stats=None):
    """One line: (record without first_part as a tuple: cost, n_chars, n_breaks, n_sub, n_del, n_ins, n_parts; labels; sources;
    parts; word_of_part).  stats (a dict or None) counts what the returned path takes."""
    R = len(n_cuts)
    if R > MAX_RUNS:
        return (-1, 0, 0, 0, 0, 0, 0), [], [], [], []
    L = LR.Word(n_cuts, first_piece, run_rows, piece_rows, first_run, n)
    B = np.asarray(B, np.int64).reshape(n + 1, n + 1)
    G = np.asarray(gaps, np.int64).reshape(-1, 2)
    E = n
    V = [np.full(n + 1, INF, np.int64)]
    V[0][E] = 0
    steps = [None]                                         # per node >= 1: (run, j, move, i, pred, is_ins, ins_pred, teq)
    brk = []                                               # per run: the state the break in front of it comes from (-1: a join)
    even = []                                              # per run: join and break cost the same at E (the join stays)
    top = 0
    for r, A in enumerate(L.atoms):
        come, same = -1, False
        if r > 0:                                          # the gap step of str_er_line_decode, on V at the run's local node 0
            J, K = int(G[first_run + r, 0]), int(G[first_run + r, 1])
            v = V[L.off[r]]
            W = np.full(n + 1, INF, np.int64) if J == OFF else v + J
            if K != OFF:
                end = v + B[:, E]
                a = int(np.argmin(end))                    # (numpy: the first of equal minima)
                same = int(end[a]) + K == W[E] < INF
                if int(end[a]) + K < W[E]:
                    W[E] = int(end[a]) + K
                    come = a
            V[L.off[r]] = W
        brk.append(come); even.append(same)
        for j in range(1, A + 1):                          # the node step of str_er_lattice_decode
            U = np.full(n + 1, INF, np.int64)
            move = np.zeros(n + 1, np.int64)
            frm = np.zeros(n + 1, np.int64)
            pred = np.zeros(n + 1, np.int64)
            teq = np.zeros(n + 1, bool)                    # a later edge costs what the kept move costs
            for i in range(j):
                Vf = V[L.off[r] + i]
                s = split if i > 0 else 0
                cand = Vf[:, None] + B[:, :n]              # [a, b]
                S = cand.min(axis=0) + L.rows[r, i, j] + s
                a = cand.argmin(axis=0)
                better = S < U[:n]
                teq[:n] = np.where(better, False, teq[:n] | ((S == U[:n]) & (S < INF)))
                U[:n] = np.where(better, S, U[:n])
                move[:n] = np.where(better, SUB, move[:n]); frm[:n] = np.where(better, i, frm[:n]); pred[:n] = np.where(better, a, pred[:n])
                if dele > 0:
                    D = Vf + dele + s
                    better = D < U
                    teq = np.where(better, False, teq | ((D == U) & (D < INF) & (i > 0)))
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
            top = max(top, int(W.max()))
            steps.append((r, j, move, frm, pred, is_ins, ins_pred, teq))
    end = V[L.N] + B[:, E]
    state = int(np.argmin(end))
    cost = int(end[state])
    assert cost < INF and top < (1 << 25)                  # (INF is never the minimum; every value is below 2^25)
    labels, src, parts, wop = [], [], [], []
    n_sub = n_del = n_ins = n_brk = 0
    node = L.N
    while node > 0:
        r, j, move, frm, pred, is_ins, ins_pred, teq = steps[node]
        k = len(parts)                                     # (counted from the end until the number of parts is known)
        if is_ins[state]:
            labels.append(state); src.append((k, SRC_INS)); n_ins += 1
            state = int(ins_pred[state])
        i = int(frm[state])
        parts.append(L.part[r, i, j])
        if stats is not None and i > 0:
            stats["i%d" % i] = stats.get("i%d" % i, 0) + 1
        if stats is not None and i == 0 and teq[state]:    # the unsplit reading kept against a split one of the same cost
            stats["tie_split"] = stats.get("tie_split", 0) + 1
        if move[state] == DEL:
            n_del += 1
            wop.append(-1)
        else:
            labels.append(state); src.append((k, 0)); n_sub += 1
            wop.append(n_brk)                              # (the breaks behind it; turned round below)
            state = int(pred[state])
        if stats is not None and i == 0 and state == E and even[r]:
            stats["tie_gap"] = stats.get("tie_gap", 0) + 1
        if i == 0 and state == E and brk[r] >= 0:          # local node 0 of a run reached at the boundary behind a break
            labels.append(E); src.append((k, SRC_BREAK)); n_brk += 1
            if stats is not None and brk[r] == E:
                stats["break_from_E"] = stats.get("break_from_E", 0) + 1
            state = brk[r]
        node = L.off[r] + i
    assert state == E
    labels.reverse(); src.reverse(); parts.reverse(); wop.reverse()
    src = [(len(parts) - 1 - k) | flag for k, flag in src]
    wop = [n_brk - v if v >= 0 else -1 for v in wop]
    if stats is not None:
        for key, v in (("break", n_brk), ("del", n_del), ("ins", n_ins), ("lines", 1)):
            stats[key] = stats.get(key, 0) + v
    return (cost, len(labels), n_brk, n_sub, n_del, n_ins, len(parts)), labels, src, parts, wop


def node_slots(splits):
    """The node slot of every run (and, last, the atoms of all runs): the atoms of the runs before it."""
    return np.concatenate([[0], np.cumsum([int(s["n_cuts"]) + 1 for s in splits])]).astype(np.int64)


def decode_lines(splits, run_costs, piece_costs, gaps, first_run, n_of, B, ins=0, dele=0, split=8, n=65, stats=None):
    """Every line of a call (splits: records with n_cuts and first_piece): the records as tuples in the order of FIELDS, chars (3 S,)
    uint8 and src (3 S,) uint16 with S the atoms of all runs, 0xFF / 0xFFFF where nothing is written, the parts as an (n_parts, 2)
    int32 array and word_of_part (n_parts,) int32."""
    slot = node_slots(splits)
    S = int(slot[-1])
    recs, parts, wop = [], [], []
    chars = np.full(3 * S, 0xFF, np.uint8)
    src = np.full(3 * S, 0xFFFF, np.uint16)
    for f, k in zip(first_run, n_of):
        f, k = int(f), max(0, int(k))
        cuts = [int(splits[r]["n_cuts"]) for r in range(f, f + k)]
        fps = [int(splits[r]["first_piece"]) for r in range(f, f + k)]
        rec, lab, s, pt, wp = decode_line(cuts, fps, run_costs, piece_costs, gaps, B, ins, dele, split, f, n, stats)
        recs.append(rec[:6] + (len(parts), rec[6]))
        parts += pt
        wop += wp
        at = 3 * int(slot[f])
        chars[at:at + len(lab)] = lab
        src[at:at + len(s)] = s
    return recs, chars, src, np.asarray(parts, np.int32).reshape(-1, 2), np.asarray(wop, np.int32)


def enumerate_best(n_cuts, first_piece, run_rows, piece_rows, gaps, B, ins, dele, split, n):
    """The cheapest of every path, by brute force: per run every segmentation, per edge one of DEL, SUB b, or either followed by one
    inserted character c (after some character), per gap a join (J on) or a break (K on).  A run's paths, strings and moves are all
    walked from every state the gap in front of it can leave -- the runs meet in that state alone -- and the minimum is kept per state."""
    L = LR.Word(n_cuts, first_piece, run_rows, piece_rows, 0, n)
    B = np.asarray(B, np.int64).reshape(n + 1, n + 1)
    G = np.asarray(gaps, np.int64).reshape(-1, 2)
    moves = ([("del",)] if dele > 0 else []) + [("sub", b) for b in range(n)]
    if ins > 0:
        moves += [("subins", b, c) for b in range(n) for c in range(n)]
        if dele > 0:
            moves += [("delins", c) for c in range(n)]
    best = {n: 0}
    for r, A in enumerate(L.atoms):
        if r > 0:
            J, K = int(G[r, 0]), int(G[r, 1])
            gapped = {}
            for prev, c in best.items():
                for to, v in (((prev, c + J),) if J != OFF else ()) + (((n, c + int(B[prev, n]) + K),) if K != OFF else ()):
                    if to not in gapped or v < gapped[to]:
                        gapped[to] = v
            best = gapped
        nxt = {}
        for seg in LR.segmentations(A):
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


def path_cost(word, gaps, B, labels, src, parts, ins, dele, split, n=65, first_run=0):
    """The cost of a returned path and string under the definition: every part is read once or dropped, an inserted character pays INS,
    a part that does not begin its run pays SPLIT, a blank ends a word and pays the K of the gap in front of its part, every other gap
    its J.  word: a lattice_decode_ref.Word of the line's runs; parts as (run, piece) of the tables."""
    B = np.asarray(B, np.int64).reshape(n + 1, n + 1)
    G = np.asarray(gaps, np.int64).reshape(-1, 2)
    edge = {v: k for k, v in word.part.items()}
    keys = [edge[tuple(p)] for p in parts]
    s = sum(split for r, i, j in keys if i > 0)
    node = 0
    for r, i, j in keys:                                   # the parts are a path: each begins where the one before ended
        assert word.off[r] + i == node
        node = word.off[r] + j
    assert node == word.N
    prev, used, broken = n, set(), set()
    for a, t in zip(labels, src):
        s += int(B[prev, a])
        p = t & 0x3FFF
        if t & SRC_BREAK:
            r, i, j = keys[p]
            assert a == n and i == 0 and r > 0 and r not in broken       # a blank stands in front of the first part of a later run
            s += int(G[first_run + r, 1]); broken.add(r)
        elif t & SRC_INS:
            s += ins
        else:
            s += int(word.rows[keys[p]][a]); used.add(p)
        prev = a
    s += sum(int(G[first_run + r, 0]) for r in range(1, len(word.atoms)) if r not in broken)
    return s + int(B[prev, n]) + dele * (len(parts) - len(used))


def as_tuples(recs) -> list:
    """The library's LINE_LATTICE_DECODE_DTYPE records as tuples in the order of FIELDS."""
    return [tuple(int(r[k]) for k in FIELDS) for r in recs]
