"""A numpy reference of the lattice decoder's margins (str_er_lattice_margin in include/str_er.h), written from the definition: the
min-marginals of the recurrence of str_er_lattice_decode -- for every edge of a word's lattice and every reading of it (a label, or
n: the edge dropped) the cost of the cheapest whole path that takes the edge and reads it that way -- by a backward pass beside the
forward one, and from them the reading margin and the cut margin of every part of the decoded path and of the word.  Beside it an
enumeration of every path through the lattice with every string and every choice of moves (the walk of
lattice_decode_ref.enumerate_best, carried whole so that a minimum can be kept per (edge, reading) and per part sequence), for small
alphabets.  The alphabet size is a parameter: the library's is 65, the boundary symbol is E = n."""
import itertools

import numpy as np

import lattice_decode_ref as LD

INF = LD.INF
MAX_NODES = LD.MAX_NODES
MARGIN_FIELDS = ("read_margin", "read_part", "read", "alt", "cut_margin", "cut_part", "cut_alt", "n_edges")
NONE_RECORD = (-1, -1, -1, -1, -1, -1, -1, 0)


def _forward(L, B, ins, dele, split, n):
    """The decoder's forward values V_0 .. V_N (after INS) of the lattice L."""
    V = [np.full(n + 1, INF, np.int64)]
    V[0][n] = 0
    for r, A in enumerate(L.atoms):
        for j in range(1, A + 1):
            U = np.full(n + 1, INF, np.int64)
            for i in range(j):
                Vf = V[L.off[r] + i]
                s = split if i > 0 else 0
                U[:n] = np.minimum(U[:n], (Vf[:, None] + B[:, :n]).min(axis=0) + L.rows[r, i, j] + s)
                if dele > 0:
                    U = np.minimum(U, Vf + dele + s)
            W = U.copy()
            if ins > 0:
                W[:n] = np.minimum(U[:n], (U[:n, None] + B[:n, :n]).min(axis=0) + ins)
            V.append(W)
    return V


def edge_marginals(L, B, ins=0, dele=0, split=8, n=65):
    """(cost, M): M[(r, i, j)] the n + 1 marginals of that edge, -1 where no path exists; the backward form of the definition."""
    B = np.asarray(B, np.int64).reshape(n + 1, n + 1)
    E, N = n, L.N
    V = _forward(L, B, ins, dele, split, n)
    cost = int((V[N] + B[:, E]).min())
    G = {N: B[:, E].copy()}
    GU = {}
    M = {}
    for r in range(len(L.atoms) - 1, -1, -1):
        A, off = L.atoms[r], L.off[r]
        for i in range(A, -1, -1):
            f = off + i
            if i < A:                                            # G_f from the edges that leave local node i
                s = split if i > 0 else 0
                H = np.min([L.rows[r, i, j] + GU[off + j][:n] for j in range(i + 1, A + 1)], axis=0)
                G[f] = (B[:, :n] + H[None, :]).min(axis=1) + s
                if dele > 0:
                    G[f] = np.minimum(G[f], dele + s + np.min([GU[off + j] for j in range(i + 1, A + 1)], axis=0))
            through = int((V[f] + G[f]).min())
            assert through >= cost and (i not in (0, A) or through == cost)          # equal at every run boundary
            if i == 0:
                break                                            # (GU and the edges into the boundary belong to the run before)
            g = G[f].copy()
            if ins > 0:
                g[:n] = np.minimum(g[:n], (B[:n, :n] + G[f][None, :n]).min(axis=1) + ins)
            GU[f] = g
    for (r, i, j), row in L.rows.items():
        f, t = L.off[r] + i, L.off[r] + j
        s = split if i > 0 else 0
        m = np.full(n + 1, -1, np.int64)
        m[:n] = (V[f][:, None] + B[:, :n]).min(axis=0) + row + s + GU[t][:n]
        if dele > 0:
            m[E] = int((V[f] + dele + s + GU[t]).min())
        M[r, i, j] = np.where(m >= INF, -1, m)
    assert N == 0 or int(G[0][E]) == cost
    return cost, M


def _moves(ins, dele, n):
    moves = ([("del",)] if dele > 0 else []) + [("sub", b) for b in range(n)]
    if ins > 0:
        moves += [("subins", b, c) for b in range(n) for c in range(n)]
        if dele > 0:
            moves += [("delins", c) for c in range(n)]
    return moves


def enumerate_paths(L, B, ins, dele, split, n):
    """Every whole path of the lattice with every string and every choice of moves along it, by brute force (the walk of
    lattice_decode_ref.enumerate_best, the runs carried together): (cost, M, S) with M[(r, i, j)] the minimum per reading of that edge
    over the paths that take it (-1: none) and S[part sequence] the minimum over the paths with that sequence of edges."""
    B = np.asarray(B, np.int64).reshape(n + 1, n + 1)
    moves = _moves(ins, dele, n)
    M = {e: np.full(n + 1, -1, np.int64) for e in L.rows}
    S = {}
    for segs in itertools.product(*[LD.segmentations(A) for A in L.atoms]):
        edges = tuple((r, i, j) for r, seg in enumerate(segs) for i, j in seg)
        for path in itertools.product(moves, repeat=len(edges)):
            prev, s, ok = n, 0, True
            for e, mv in zip(edges, path):
                s += split if e[1] > 0 else 0
                if mv[0] == "del":
                    s += dele
                elif mv[0] == "sub":
                    s += int(B[prev, mv[1]]) + int(L.rows[e][mv[1]]); prev = mv[1]
                elif mv[0] == "subins":
                    s += int(B[prev, mv[1]]) + int(L.rows[e][mv[1]]) + int(B[mv[1], mv[2]]) + ins; prev = mv[2]
                else:
                    if prev == n:                                # only after some character
                        ok = False
                        break
                    s += dele + int(B[prev, mv[1]]) + ins; prev = mv[1]
            if not ok:
                continue
            s += int(B[prev, n])
            if edges not in S or s < S[edges]:
                S[edges] = s
            for e, mv in zip(edges, path):
                x = mv[1] if mv[0] in ("sub", "subins") else n
                if M[e][x] < 0 or s < M[e][x]:
                    M[e][x] = s
    return min(S.values()), M, S


def edge_min(m):
    """m_e: the minimum of the marginals of an edge that exist."""
    return int(m[m >= 0].min())


def margins_word(n_cuts, first_piece, run_rows, piece_rows, B, ins=0, dele=0, split=8, first_run=0, n=65):
    """One word: a dict with the record (a tuple in the order of MARGIN_FIELDS), the per-part lists read_margin, cut_margin, read, alt,
    cut_alt, the decoded edges, the marginals M per edge, the lattice and the cost.  A word of no atoms or of more than 32: the record of -1."""
    L = LD.Word(n_cuts, first_piece, run_rows, piece_rows, first_run, n)
    none = dict(rec=NONE_RECORD, read_margin=[], cut_margin=[], read=[], alt=[], cut_alt=[], edges=[], M={}, L=L, cost=None)
    if L.N < 1 or L.N > MAX_NODES:
        return none
    rec, labels, src, parts = LD.decode_word(n_cuts, first_piece, run_rows, piece_rows, B, ins, dele, split, first_run, n)
    cost, M = edge_marginals(L, B, ins, dele, split, n)
    assert cost == rec[0]
    edge_of = {v: k for k, v in L.part.items()}
    edges = [edge_of[tuple(p)] for p in parts]
    read = [n] * len(parts)
    for a, t in zip(labels, src):
        if not t & 0x80:
            read[t] = a
    read_margin, alt, cut_margin, cut_alt = [], [], [], []
    for k, (r, i, j) in enumerate(edges):
        assert int(M[r, i, j][read[k]]) == cost
        best, x = min((int(M[r, i, j][x]), x) for x in range(n + 1) if x != read[k] and M[r, i, j][x] >= 0)
        read_margin.append(best - cost); alt.append(x)
        others = [(edge_min(M[r, a, b]), a, b) for (q, a, b) in L.rows if q == r and (a, b) != (i, j) and a < j and b > i]
        if others:
            v, a, b = min(others)                                # (the smallest (i', j') among equals)
            cut_margin.append(v - cost); cut_alt.append(a | b << 4)
        else:
            cut_margin.append(-1); cut_alt.append(0xFF)
    rm = min(read_margin)
    rp = read_margin.index(rm)
    cuts = [v for v in cut_margin if v >= 0]
    cm = min(cuts) if cuts else -1
    cp = cut_margin.index(cm) if cuts else -1
    record = (rm, rp, read[rp], alt[rp], cm, cp, cut_alt[cp] if cuts else -1, len(L.rows))
    return dict(rec=record, read_margin=read_margin, cut_margin=cut_margin, read=read, alt=alt, cut_alt=cut_alt, edges=edges, M=M, L=L, cost=cost)


def lattice_margins(splits, run_costs, piece_costs, first_run, n_of, B, ins=0, dele=0, split=8):
    """Every word at the library's alphabet, in the library's layout: the records as tuples, read_margin and cut_margin (n_words, 32)
    int32, read, alt and cut_alt (n_words, 32) uint8, edge_min (n_words, 32, 4) int32 and marginals (n_words, 32, 4, 66) int32."""
    nw = len(first_run)
    recs = []
    rm = np.full((nw, 32), -1, np.int32); cm = np.full((nw, 32), -1, np.int32)
    rd = np.full((nw, 32), 0xFF, np.uint8); al = np.full((nw, 32), 0xFF, np.uint8); ca = np.full((nw, 32), 0xFF, np.uint8)
    em = np.full((nw, 32, 4), -1, np.int32); mg = np.full((nw, 32, 4, 66), -1, np.int32)
    for w, (f, k) in enumerate(zip(first_run, n_of)):
        f, k = int(f), int(k)
        cuts = [int(splits[r]["n_cuts"]) for r in range(f, f + k)]
        fps = [int(splits[r]["first_piece"]) for r in range(f, f + k)]
        R = margins_word(cuts, fps, run_costs, piece_costs, B, ins, dele, split, f)
        recs.append(R["rec"])
        p = len(R["edges"])
        rm[w, :p] = R["read_margin"]; cm[w, :p] = R["cut_margin"]; rd[w, :p] = R["read"]; al[w, :p] = R["alt"]; ca[w, :p] = R["cut_alt"]
        for (r, i, j), m in R["M"].items():
            t = R["L"].off[r] + j
            em[w, t - 1, i] = edge_min(m)
            mg[w, t - 1, i] = m
    return recs, rm, cm, rd, al, ca, em, mg


def as_tuples(recs) -> list:
    """The library's LATTICE_MARGIN_DTYPE records as tuples in the order of MARGIN_FIELDS."""
    return [tuple(int(r[k]) for k in MARGIN_FIELDS) for r in recs]
