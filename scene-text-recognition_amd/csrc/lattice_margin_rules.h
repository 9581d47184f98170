// lattice_margin_rules.h -- INTERNAL: the rules of the lattice decoder's margins (the contract is at str_er_lattice_margin in str_er.h):
// the min-marginals of the recurrence of lattice_decode_rules.h -- for every edge of the word's lattice and every reading of it the cost
// of the cheapest whole path that takes the edge and reads it that way -- by one backward pass over the nodes beside the forward one,
// and from them the reading margin and the cut margin of every part of the decoded path and of the word.  HIP-free and header-only: the
// host entry point (api_lattice_margin.cpp: str_er_lattice_margins_host) and tests/cpp/lattice_margin_rules_check.cpp use this same
// code; lattice_margin_kernels.hip states the same rules for the device and is held against the numpy reference
// (tests/lattice_margin_ref.py), which is written from the definition.
#pragma once
#include "lattice_decode_rules.h"

namespace str_er_ld {

constexpr int MARGINALS = wd::STATES;          // per edge: the 65 readings and, at 65, the edge dropped
constexpr int MAX_FROM = 4;                    // the local nodes an edge into a node can leave: 0 .. 3
constexpr int MAX_PARTS = MAX_NODES;

// One word: the runs first_run .. first_run + n_of of splits with their rows under B with INS, DEL and SPLIT, and what the decoder made
// of them (chars / src: its 64 + 64 bytes, n_chars of them used; parts: its n_parts lattice parts, with the piece indices of the
// tables).  read_margin and cut_margin receive 32 values (-1 past n_parts), read, alt and cut_alt 32 bytes each (0xFF past n_parts);
// edge_min (null: not wanted) 32 x 4 values, [n - 1][i] of the edge from the local node i into the word's node n, and marginals
// (null: not wanted) 32 x 4 x 66 values with the same index; both -1 where there is no edge or no path.
inline str_er_lattice_margin margins_word(const str_er_run_split *splits, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t first_run, int32_t n_of,
                                          const uint8_t *B, int32_t ins, int32_t del, int32_t split, const uint8_t *chars, const uint8_t *src, int n_chars,
                                          const str_er_split_part *parts, int n_parts, int32_t *read_margin, int32_t *cut_margin, uint8_t *read, uint8_t *alt,
                                          uint8_t *cut_alt, int32_t *edge_min, int32_t *marginals)
{
    constexpr int STATES = wd::STATES, ALPHABET = wd::ALPHABET, E = wd::E;
    constexpr int32_t INF = wd::INF;
    str_er_lattice_margin R{-1, -1, -1, -1, -1, -1, -1, 0};
    for (int k = 0; k < MAX_PARTS; ++k) { read_margin[k] = cut_margin[k] = -1; read[k] = alt[k] = cut_alt[k] = 0xFF; }
    if (edge_min)
        for (int t = 0; t < MAX_NODES * MAX_FROM; ++t) edge_min[t] = -1;
    if (marginals)
        for (int t = 0; t < MAX_NODES * MAX_FROM * MARGINALS; ++t) marginals[t] = -1;
    const int64_t N64 = word_nodes(splits, first_run, n_of);
    if (N64 < 1 || N64 > MAX_NODES || n_parts < 1 || n_parts > MAX_PARTS) return R;
    const int N = (int)N64;
    // the nodes: node n >= 1 is the local node node_j[n] of run node_run[n]; node_off[n] is the word's node of that run's local node 0
    int32_t node_run[MAX_NODES + 1], node_j[MAX_NODES + 1], node_off[MAX_NODES + 1], node_A[MAX_NODES + 1];
    {
        int n = 0;
        for (int32_t run = first_run; run < first_run + n_of; ++run) {
            const int A = splits[run].n_cuts + 1, off = n;
            for (int j = 1; j <= A; ++j) { ++n; node_run[n] = run; node_j[n] = j; node_off[n] = off; node_A[n] = A; }
            R.n_edges += A * (A + 1) / 2;
        }
    }
    const auto row_of = [&](int n, int i) {          // the row of the edge from the local node i into node n
        const str_er_run_split &S = splits[node_run[n]];
        const int k = rs::piece_index(node_A[n], i, node_j[n]);
        return k < 0 ? run_costs + (size_t)node_run[n] * ALPHABET : piece_costs + ((size_t)S.first_piece + (size_t)k) * ALPHABET;
    };
    // the forward pass of decode_word without its moves: every V_n and P_n[b] = min over a of V_n[a] + B[a][b]
    int32_t V[MAX_NODES + 1][STATES], P[MAX_NODES][ALPHABET], U[STATES];
    for (int a = 0; a < ALPHABET; ++a) V[0][a] = INF;
    V[0][E] = 0;
    for (int n = 1; n <= N; ++n) {
        {
            const int32_t *Vf = V[n - 1];
            for (int b = 0; b < ALPHABET; ++b) {
                int32_t best = Vf[0] + B[b];
                for (int a = 1; a < STATES; ++a) best = Vf[a] + B[a * STATES + b] < best ? Vf[a] + B[a * STATES + b] : best;
                P[n - 1][b] = best;
            }
        }
        for (int x = 0; x < STATES; ++x) U[x] = INF;
        for (int i = 0; i < node_j[n]; ++i) {
            const int      f = node_off[n] + i;
            const uint8_t *row = row_of(n, i);
            const int32_t  s = i > 0 ? split : 0;
            for (int b = 0; b < ALPHABET; ++b)
                if (P[f][b] + row[b] + s < U[b]) U[b] = P[f][b] + row[b] + s;
            if (del > 0)
                for (int a = 0; a < STATES; ++a)
                    if (V[f][a] + del + s < U[a]) U[a] = V[f][a] + del + s;
        }
        for (int c = 0; c < STATES; ++c) V[n][c] = U[c];
        if (ins > 0)
            for (int c = 0; c < ALPHABET; ++c) {
                int32_t best = U[0] + B[c];
                for (int b = 1; b < ALPHABET; ++b) best = U[b] + B[b * STATES + c] < best ? U[b] + B[b * STATES + c] : best;
                if (best + ins < U[c]) V[n][c] = best + ins;
            }
    }
    int32_t cost = V[N][0] + B[E];
    for (int a = 1; a < STATES; ++a) cost = V[N][a] + B[a * STATES + E] < cost ? V[N][a] + B[a * STATES + E] : cost;
    // the decoded path: the in-edge of its end node and its reading, per part
    int     part_n[MAX_PARTS], part_i[MAX_PARTS];
    uint8_t x[MAX_PARTS];
    {
        int n = 0;
        for (int k = 0; k < n_parts; ++k) {
            if (n >= N) return str_er_lattice_margin{-1, -1, -1, -1, -1, -1, -1, 0};          // (not a path of this word)
            const int32_t run = node_run[n + 1], A = node_A[n + 1], kk = parts[k].piece < 0 ? -1 : parts[k].piece - splits[run].first_piece;
            int           pi = -1, pj = -1;
            for (int i = 0; i < A; ++i)
                for (int j = i + 1; j <= A; ++j)
                    if (rs::piece_index(A, i, j) == kk) { pi = i; pj = j; }
            if (parts[k].run != run || pi < 0 || node_off[n + 1] + pi != n) return str_er_lattice_margin{-1, -1, -1, -1, -1, -1, -1, 0};
            n = node_off[n + 1] + pj;
            part_n[k] = n; part_i[k] = pi;
            x[k] = (uint8_t)E;
        }
        for (int t = 0; t < n_chars && t < MAX_CHARS; ++t)
            if (!(src[t] & 0x80) && src[t] < n_parts) x[src[t]] = chars[t];
    }
    // the backward pass over the nodes N .. 1: GU_n, the marginals of the edges into n, and H and the DEL term of the nodes they leave
    int32_t G[STATES], GU[STATES], H[MAX_FROM][ALPHABET], D[MAX_FROM][STATES], M[MARGINALS], em[MAX_NODES][MAX_FROM];
    for (int n = 0; n < MAX_NODES; ++n)
        for (int i = 0; i < MAX_FROM; ++i) em[n][i] = -1;
    for (int a = 0; a < STATES; ++a) G[a] = B[a * STATES + E];
    for (int n = N; n >= 1; --n) {
        const int j = node_j[n], A = node_A[n], off = node_off[n];
        if (j == A)          // the last node of its run: nothing leaves the run's local nodes yet
            for (int i = 0; i < MAX_FROM; ++i) {
                for (int b = 0; b < ALPHABET; ++b) H[i][b] = 4 * INF;
                for (int a = 0; a < STATES; ++a) D[i][a] = 4 * INF;
            }
        for (int a = 0; a < STATES; ++a) GU[a] = G[a];
        if (ins > 0)
            for (int b = 0; b < ALPHABET; ++b) {
                int32_t best = B[b * STATES] + G[0];
                for (int c = 1; c < ALPHABET; ++c) best = B[b * STATES + c] + G[c] < best ? B[b * STATES + c] + G[c] : best;
                if (best + ins < GU[b]) GU[b] = best + ins;
            }
        for (int i = 0; i < j; ++i) {
            const int      f = off + i;
            const uint8_t *row = row_of(n, i);
            const int32_t  s = i > 0 ? split : 0;
            for (int b = 0; b < ALPHABET; ++b) {
                M[b] = P[f][b] + row[b] + s + GU[b];
                if (row[b] + GU[b] < H[i][b]) H[i][b] = row[b] + GU[b];
            }
            M[E] = -1;
            if (del > 0) {
                int32_t best = V[f][0] + del + s + GU[0];
                for (int a = 1; a < STATES; ++a) best = V[f][a] + del + s + GU[a] < best ? V[f][a] + del + s + GU[a] : best;
                M[E] = best;
                for (int a = 0; a < STATES; ++a)
                    if (GU[a] < D[i][a]) D[i][a] = GU[a];
            }
            int32_t least = -1;
            for (int k = 0; k < MARGINALS; ++k) {
                if (M[k] >= INF) M[k] = -1;          // (no path: INF never wins)
                if (M[k] >= 0 && (least < 0 || M[k] < least)) least = M[k];
            }
            em[n - 1][i] = least;
            if (marginals)
                for (int k = 0; k < MARGINALS; ++k) marginals[((n - 1) * MAX_FROM + i) * MARGINALS + k] = M[k];
            for (int k = 0; k < n_parts; ++k)
                if (part_n[k] == n && part_i[k] == i) {          // the edge is part k of the path: its reading margin
                    int32_t best = -1;
                    int     at = -1;
                    for (int y = 0; y < MARGINALS; ++y)
                        if (y != x[k] && M[y] >= 0 && (best < 0 || M[y] < best)) { best = M[y]; at = y; }
                    read_margin[k] = best - cost; read[k] = x[k]; alt[k] = (uint8_t)at;
                }
        }
        // G of the node before: the local node j - 1 of this run, whose edges have all been seen
        const int     i = j - 1;
        const int32_t s = i > 0 ? split : 0;
        for (int a = 0; a < STATES; ++a) {
            int32_t nb = B[a * STATES] + H[i][0];
            for (int b = 1; b < ALPHABET; ++b) nb = B[a * STATES + b] + H[i][b] < nb ? B[a * STATES + b] + H[i][b] : nb;
            nb += s;
            if (del > 0 && del + s + D[i][a] < nb) nb = del + s + D[i][a];
            G[a] = nb;
        }
    }
    if (edge_min)
        for (int n = 0; n < MAX_NODES; ++n)
            for (int i = 0; i < MAX_FROM; ++i) edge_min[n * MAX_FROM + i] = em[n][i];
    // the cut margin of every part: the other edges of its run over its atoms
    for (int k = 0; k < n_parts; ++k) {
        const int n = part_n[k], off = node_off[n], A = node_A[n], jk = node_j[n], ik = part_i[k];
        for (int i = 0; i < A; ++i)
            for (int j = i + 1; j <= A; ++j) {
                if ((i == ik && j == jk) || i >= jk || j <= ik) continue;
                const int32_t v = em[off + j - 1][i] - cost;
                if (cut_margin[k] < 0 || v < cut_margin[k]) { cut_margin[k] = v; cut_alt[k] = (uint8_t)(i | j << 4); }
            }
    }
    for (int k = 0; k < n_parts; ++k) {
        if (R.read_margin < 0 || read_margin[k] < R.read_margin) { R.read_margin = read_margin[k]; R.read_part = k; R.read = read[k]; R.alt = alt[k]; }
        if (cut_margin[k] >= 0 && (R.cut_margin < 0 || cut_margin[k] < R.cut_margin)) { R.cut_margin = cut_margin[k]; R.cut_part = k; R.cut_alt = cut_alt[k]; }
    }
    return R;
}

} // namespace str_er_ld
