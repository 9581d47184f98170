"""A numpy reference of the line decoder's margins (str_er_line_margin in include/str_er.h), written from the definition: the forward
values V_{i-1}, W_i, X_i and S_i of the line decoder's recurrence, the backward values G, GU and H, the row marginals and the gap
marginals, the readings from the decoded string (line_decode_ref.decode_line) and the margins, and an enumeration of every path (the
one of line_decode_ref.enumerate_best) that records the cheapest path per (row, reading) and per (gap, move) for small alphabets.  The
alphabet size is a parameter: the library's is 65; E = n."""
import itertools

import numpy as np

import line_decode_ref as LD

INF = LD.INF
OFF = LD.OFF
MAX_ROWS = LD.MAX_ROWS
MARGIN_FIELDS = ("margin", "read_margin", "row", "read", "alt", "gap_margin", "gap", "gap_move")
NO_MARGIN = (-1,) * 8


def _arrays(C, G, B, n):
    return np.asarray(C, np.int64).reshape(-1, n), np.asarray(G, np.int64).reshape(-1, 2), np.asarray(B, np.int64).reshape(n + 1, n + 1)


def _clean(v):
    return np.where(np.asarray(v) >= INF, -1, v)


def marginals_backward(C, G, B, ins=0, dele=0, n=65):
    """(cost, M (m, n + 1), MG (m, 2): join and break of the gap in front of every row), -1 where there is none."""
    C, G, B = _arrays(C, G, B, n)
    m, E = len(C), n
    # forward: V_{i-1}, W_i, X_i, S_i
    Vs, Ws, Xs, Ss = [], [], [], []
    V = np.full(n + 1, INF, np.int64)
    V[E] = 0
    for i in range(1, m + 1):
        Vs.append(V.copy())
        X = None
        W = V.copy()
        if i >= 2:
            J, K = int(G[i - 1, 0]), int(G[i - 1, 1])
            W = np.full(n + 1, INF, np.int64) if J == OFF else V + J
            if K != OFF:
                X = int((V + B[:, E]).min()) + K
                W[E] = min(int(W[E]), X)
        Ws.append(W); Xs.append(X)
        S = (W[:, None] + B[:, :n]).min(axis=0) + C[i - 1]
        Ss.append(S)
        U = np.full(n + 1, INF, np.int64)
        U[:n] = S
        if dele > 0:
            U = np.minimum(U, W + dele)
        V = U.copy()
        if ins > 0:
            V[:n] = np.minimum(U[:n], (U[:n, None] + B[:n, :n]).min(axis=0) + ins)
    cost = int((V + B[:, E]).min())
    # backward
    M = np.full((m, n + 1), -1, np.int64)
    MG = np.full((m, 2), -1, np.int64)
    Gb = B[:, E].copy()
    for i in range(m, 0, -1):
        GU = Gb.copy()
        if ins > 0:
            GU[:n] = np.minimum(Gb[:n], (B[:n, :n] + Gb[None, :n]).min(axis=1) + ins)
        H = (B[:, :n] + (C[i - 1] + GU[:n])[None, :]).min(axis=1)
        if dele > 0:
            H = np.minimum(H, dele + GU)
        M[i - 1, :n] = Ss[i - 1] + GU[:n]
        if dele > 0:
            M[i - 1, E] = int((Ws[i - 1] + dele + GU).min())
        if i >= 2:
            J, K = int(G[i - 1, 0]), int(G[i - 1, 1])
            cands = []
            if J != OFF:
                MG[i - 1, 0] = int((Vs[i - 1] + J + H).min())
                cands.append(J + H)
            if K != OFF:
                MG[i - 1, 1] = Xs[i - 1] + int(H[E])
                cands.append(B[:, E] + K + int(H[E]))
            Gb = np.minimum.reduce(cands)
        else:
            Gb = H
    assert m == 0 or int(Gb[E]) == cost
    return cost, _clean(M), _clean(MG)


def marginals_enumerated(C, G, B, ins, dele, n):
    """The same by brute force: the enumeration of line_decode_ref.enumerate_best, recording per row what it does there (read as b:
    b, dropped: n) and per gap its move."""
    C, G, B = _arrays(C, G, B, n)
    m = len(C)
    moves = ([("del",)] if dele > 0 else []) + [("sub", b) for b in range(n)]
    if ins > 0:
        moves += [("subins", b, c) for b in range(n) for c in range(n)]
        if dele > 0:
            moves += [("delins", c) for c in range(n)]
    M = np.full((m, n + 1), -1, np.int64)
    MG = np.full((m, 2), -1, np.int64)
    best = None
    for gaps in itertools.product((0, 1), repeat=max(0, m - 1)):
        if any(int(G[i + 1, g]) == OFF for i, g in enumerate(gaps)):
            continue
        gsum = sum(int(G[i + 1, g]) for i, g in enumerate(gaps))
        for path in itertools.product(moves, repeat=m):
            prev, s, ok = n, gsum, True
            for i, mv in enumerate(path):
                if i >= 1 and gaps[i - 1] == 1:
                    s += int(B[prev, n]); prev = n
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
            best = s if best is None or s < best else best
            for i, mv in enumerate(path):
                x = mv[1] if mv[0] in ("sub", "subins") else n
                if M[i, x] < 0 or s < M[i, x]:
                    M[i, x] = s
                if i >= 1 and (MG[i, gaps[i - 1]] < 0 or s < MG[i, gaps[i - 1]]):
                    MG[i, gaps[i - 1]] = s
    return best, M, MG


def readings(m, labels, src, n=65):
    """(x_i, d_i) of every row from a decoded string: d of the first row is -1."""
    read, move = [n] * m, [-1] + [0] * (m - 1) if m else []
    for a, r in zip(labels, src):
        if not r & (LD.SRC_INS | LD.SRC_BREAK):
            read[r] = a
        elif r & LD.SRC_BREAK:
            move[r & 0x3FFF] = 1
    return read, move


def margins_line(C, G, B, ins=0, dele=0, n=65):
    """One line: (record as a tuple in the order of MARGIN_FIELDS, row_margin, row_read, row_alt, gap_margin, gap_move (-1: none),
    marginals (m, n + 3): M, then join and break, cost).  A line of no rows or of more than 1024: the record of -1 and nothing else."""
    C, G, B = _arrays(C, G, B, n)
    m = len(C)
    if m < 1 or m > MAX_ROWS:
        return NO_MARGIN, [], [], [], [], [], np.zeros((0, n + 3), np.int64), None
    rec, labels, src, wor = LD.decode_line(C, G, B, ins, dele, n)
    cost, M, MG = marginals_backward(C, G, B, ins, dele, n)
    assert cost == rec[0]
    read, move = readings(m, labels, src, n)
    row_margin, row_alt, gap_margin = [], [], []
    for i in range(m):
        assert M[i, read[i]] == cost
        best, alt = min((int(M[i, x]), x) for x in range(n + 1) if x != read[i] and M[i, x] >= 0)          # (the smallest x among equals)
        row_margin.append(best - cost)
        row_alt.append(alt)
        if i == 0:
            gap_margin.append(-1)
        else:
            assert MG[i, move[i]] == cost
            other = int(MG[i, 1 - move[i]])
            gap_margin.append(other - cost if other >= 0 else -1)
    rmin = min(row_margin)
    row = row_margin.index(rmin)
    have = [g for g in gap_margin if g >= 0]
    gmin = min(have) if have else -1
    gap = gap_margin.index(gmin) if have else -1
    margin = gmin if have and gmin < rmin else rmin
    record = (margin, rmin, row, read[row], row_alt[row], gmin, gap, move[gap] if have else -1)
    return record, row_margin, read, row_alt, gap_margin, move, np.concatenate([M, MG], axis=1), cost


def line_margins(costs, gaps, first_row, n_of, B, ins=0, dele=0):
    """Every line at the library's alphabet, in the library's layout: the records as tuples, row_margin (rows,) int32, row_read and
    row_alt (rows,) uint8, gap_margin (rows,) int32, gap_move (rows,) uint8 and the marginals (rows, 68) int32; -1 / 0xFF where nothing
    is written."""
    costs = np.asarray(costs, np.uint8).reshape(-1, 65)
    gaps = np.asarray(gaps, np.uint8).reshape(-1, 2)
    nr = len(costs)
    recs = []
    rm, gm = np.full(nr, -1, np.int32), np.full(nr, -1, np.int32)
    rr, ra, gv = np.full(nr, 0xFF, np.uint8), np.full(nr, 0xFF, np.uint8), np.full(nr, 0xFF, np.uint8)
    mg = np.full((nr, 68), -1, np.int32)
    for f, k in zip(first_row, n_of):
        f, k = int(f), max(0, int(k))
        rec, a, b, c, d, e, M, _ = margins_line(costs[f:f + k], gaps[f:f + k], B, ins, dele)
        recs.append(rec)
        if len(a):
            rm[f:f + k], rr[f:f + k], ra[f:f + k], gm[f:f + k] = a, b, c, d
            gv[f:f + k] = [0xFF if v < 0 else v for v in e]
            mg[f:f + k] = M
    return recs, rm, rr, ra, gm, gv, mg


def as_tuples(recs) -> list:
    """The library's LINE_MARGIN_DTYPE records as tuples in the order of MARGIN_FIELDS."""
    return [tuple(int(r[k]) for k in MARGIN_FIELDS) for r in recs]
