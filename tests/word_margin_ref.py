"""A numpy reference of the word decoder's margins (str_er_word_margin in include/str_er.h), written from the definition: the
min-marginals of the decoder's recurrence -- for every run and every reading of it (a label, or n: the run dropped) the cost of the
cheapest whole path that reads the run that way -- and from them the margin of every row and of the word.  Two forms: the backward
pass of the definition, and an independent one, a forward pass with one row forced to one reading; for small alphabets an enumeration
of every path beside them.  The alphabet size is a parameter, as in word_decode_ref.py: the library's is 65, E = n."""
import itertools

import numpy as np

import word_decode_ref as WD

INF = WD.INF
MAX_RUNS = WD.MAX_RUNS
MARGIN_FIELDS = ("margin", "row", "read", "alt")


def _arrays(C, B, n):
    return np.asarray(C, np.int64).reshape(-1, n), np.asarray(B, np.int64).reshape(n + 1, n + 1)


def _forward(C, B, ins, dele, n, force=None):
    """The decoder's forward pass: V_0 .. V_m and S_1 .. S_m.  force = (i, x): run i (1-based) takes the reading x alone -- SUB to x,
    or for x = n the drop -- whatever is inserted behind it."""
    m, E = len(C), n
    V = np.full(n + 1, INF, np.int64)
    V[E] = 0
    Vs, Ss = [V], []
    for i in range(1, m + 1):
        S = (V[:, None] + B[:, :n]).min(axis=0) + C[i - 1]
        U = np.full(n + 1, INF, np.int64)
        U[:n] = S
        D = V + dele if dele > 0 else np.full(n + 1, 4 * INF, np.int64)
        if force is not None and force[0] == i:
            x = force[1]
            if x == E:
                U = D.copy()
            else:
                U = np.full(n + 1, 4 * INF, np.int64)
                U[x] = S[x]
        else:
            U = np.minimum(U, D)
        W = U.copy()
        if ins > 0:
            W[:n] = np.minimum(U[:n], (U[:n, None] + B[:n, :n]).min(axis=0) + ins)
        V = W
        Vs.append(V)
        Ss.append(S)
    return Vs, Ss


def _clean(M):
    return np.where(M >= INF, -1, M)


def marginals_backward(C, B, ins=0, dele=0, n=65):
    """(cost, M): M (m, n + 1), the backward form of the definition; -1 where no path exists."""
    C, B = _arrays(C, B, n)
    m, E = len(C), n
    Vs, Ss = _forward(C, B, ins, dele, n)
    cost = int((Vs[m] + B[:, E]).min())
    G = B[:, E].copy()
    M = np.full((m, n + 1), -1, np.int64)
    for i in range(m, 0, -1):
        assert int((Vs[i] + G).min()) == cost                # the invariant
        GU = G.copy()
        if ins > 0:
            GU[:n] = np.minimum(G[:n], (B[:n, :n] + G[None, :n]).min(axis=1) + ins)
        M[i - 1, :n] = Ss[i - 1] + GU[:n]
        if dele > 0:
            M[i - 1, E] = int((Vs[i - 1] + dele + GU).min())
        G = (B[:, :n] + (C[i - 1] + GU[:n])[None, :]).min(axis=1)
        if dele > 0:
            G = np.minimum(G, dele + GU)
    assert int(G[E]) == cost
    return cost, _clean(M)


def marginals_forced(C, B, ins=0, dele=0, n=65):
    """The same table from forward passes alone: one pass per (row, reading) with that row forced to that reading."""
    C, B = _arrays(C, B, n)
    m, E = len(C), n
    M = np.full((m, n + 1), -1, np.int64)
    for i in range(1, m + 1):
        for x in range(n + 1):
            if x == E and dele <= 0:
                continue
            Vs, _ = _forward(C, B, ins, dele, n, force=(i, x))
            M[i - 1, x] = int((Vs[m] + B[:, E]).min())
    return _clean(M)


def marginals_enumerated(C, B, ins, dele, n):
    """The same table by brute force over every path of word_decode_ref.enumerate_best (small alphabets)."""
    C, B = _arrays(C, B, n)
    m = len(C)
    moves = ([("del",)] if dele > 0 else []) + [("sub", b) for b in range(n)]
    if ins > 0:
        moves += [("subins", b, c) for b in range(n) for c in range(n)]
        if dele > 0:
            moves += [("delins", c) for c in range(n)]
    M = np.full((m, n + 1), -1, np.int64)
    for path in itertools.product(moves, repeat=m):
        prev, s, ok = n, 0, True
        for i, mv in enumerate(path):
            if mv[0] == "del":
                s += dele
            elif mv[0] == "sub":
                s += int(B[prev, mv[1]]) + int(C[i, mv[1]]); prev = mv[1]
            elif mv[0] == "subins":
                s += int(B[prev, mv[1]]) + int(C[i, mv[1]]) + int(B[mv[1], mv[2]]) + ins; prev = mv[2]
            else:
                if prev == n:
                    ok = False
                    break
                s += dele + int(B[prev, mv[1]]) + ins; prev = mv[1]
        if not ok:
            continue
        s += int(B[prev, n])
        for i, mv in enumerate(path):
            x = mv[1] if mv[0] in ("sub", "subins") else n
            if M[i, x] < 0 or s < M[i, x]:
                M[i, x] = s
    return M


def margins_word(C, B, ins=0, dele=0, n=65):
    """One word: (record as a tuple in the order of MARGIN_FIELDS, row_margin, row_read, row_alt, marginals (m, n + 1), cost); the
    lists have one entry per row.  A word of no rows or of more than 32: the record of -1 and nothing else."""
    C, B = _arrays(C, B, n)
    m = len(C)
    if m < 1 or m > MAX_RUNS:
        return (-1, -1, -1, -1), [], [], [], np.zeros((0, n + 1), np.int64), None
    rec, labels, src = WD.decode_word(C, B, ins, dele, n)
    cost, M = marginals_backward(C, B, ins, dele, n)
    assert cost == rec[0]
    read = [n] * m
    for a, r in zip(labels, src):
        if not r & 0x80:
            read[r] = a
    row_margin, row_alt = [], []
    for i in range(m):
        others = [(int(M[i, x]), x) for x in range(n + 1) if x != read[i] and M[i, x] >= 0]
        best, alt = min(others)                                   # (the smallest x among equals)
        row_margin.append(best - cost)
        row_alt.append(alt)
    margin = min(row_margin)
    row = row_margin.index(margin)
    return (margin, row, read[row], row_alt[row]), row_margin, read, row_alt, M, cost


def word_margins(costs, first_run, n_of, B, ins=0, dele=0):
    """Every word at the library's alphabet, in the library's layout: the records as tuples, row_margin (n_words, 32) int32, row_read
    and row_alt (n_words, 32) uint8, marginals (n_words, 32, 66) int32."""
    costs = np.asarray(costs, np.uint8).reshape(-1, 65)
    nw = len(first_run)
    recs = []
    rm = np.full((nw, 32), -1, np.int32)
    rr = np.full((nw, 32), 0xFF, np.uint8)
    ra = np.full((nw, 32), 0xFF, np.uint8)
    mg = np.full((nw, 32, 66), -1, np.int32)
    for w, (f, k) in enumerate(zip(first_run, n_of)):
        rec, a, b, c, M, _ = margins_word(costs[int(f):int(f) + int(k)], B, ins, dele)
        recs.append(rec)
        rm[w, :len(a)] = a
        rr[w, :len(b)] = b
        ra[w, :len(c)] = c
        mg[w, :len(M)] = M
    return recs, rm, rr, ra, mg


def as_tuples(recs) -> list:
    """The library's WORD_MARGIN_DTYPE records as tuples in the order of MARGIN_FIELDS."""
    return [tuple(int(r[k]) for k in MARGIN_FIELDS) for r in recs]
