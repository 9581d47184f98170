// lattice_match_device.h -- INTERNAL, device code: what the kernels of the lexicon match over the piece lattice
// (lattice_match_kernels.hip) and of the track match over the members' lattices (lattice_track_kernels.hip) share -- the order of a
// run's pieces, the edit distance of one entry over a lattice staged in LDS, and, a wave a word, the free segmentation with the nodes
// of the word and the table of one entry with its backtrack (lattice_track_decode_kernels.hip runs that table on a string's labels from
// memory).  The rules are stated for the host in lattice_match_rules.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/str_er.h"
#include "word_match_device.h"

namespace str_er {

namespace {

constexpr int LM_MAX_NODES = 32, LM_MAX_RUNS = 33;      // (33 runs: enough to see that N > 32)
constexpr int LM_SLOTS = 4 * LM_MAX_NODES;                                  // row slots in LDS: (node, span)
constexpr int LM_PIECE = 0x40000000;                                       // a slot's row: the run's row, or with this bit the piece's; -1: none
constexpr int LM_TROW = 33;                                                 // ints of a row of the final table

// the piece (i, j) of a run of A atoms in the order by (i, j) without (0, A); -1: the run itself
__device__ __forceinline__ int lm_piece_index(int A, int i, int j)
{
    if (i == 0) return j == A ? -1 : j - 1;
    return (A - 1) + (i - 1) * A - (i - 1) * i / 2 + (j - i - 1);
}

__device__ __forceinline__ int lm_atoms(const str_er_run_split *splits, int r) { return min(max(splits[r].n_cuts, 0), 3) + 1; }

// one edge into the node n (static) from D_ nodes back: the old value there (SUB) and the new one (DEL), with the edge's penalty
#define LM_EDGE(D_, OLD_, PEN_, DELPEN_)                                                          \
    {                                                                                             \
        const int c = ct[((n - 1) * 4 + (D_ - 1)) * WM_ALPHABET + a];                              \
        best = min(best, min(OLD_ + c + PEN_, col[n - D_] + DELPEN_));                            \
    }

// The edit distance of the lane's entry of `len` labels over the lattice of N <= MC nodes: jl - 1 of the node n in the bits 2 (n - 1) of
// S0 (n <= 16) or 2 (n - 17) of S1 (uniform), d0[n] = D[n][0].  Rows past N are computed and not used.  A node with jl = 1 takes the
// matcher's cell after one uniform branch; the edge that begins its run (d = jl) has no penalty, the shorter ones pay SPLIT.
template <int MC>
__device__ __forceinline__ int lm_entry_cost(const uint8_t *ct, uint32_t S0, uint32_t S1, const int *d0, const uint32_t *__restrict__ words, int len, int N, int ins,
                                             int del, int split)
{
    int       col[MC + 1];
    const int dsp = del + split;
#pragma unroll
    for (int n = 0; n <= MC; ++n) col[n] = d0[n];
    for (int q = 0; q * 4 < len; ++q) {
        const uint32_t w = words[q * WM_GROUP];
        for (int jj = 0; jj < 4 && q * 4 + jj < len; ++jj) {
            const int a = (int)(w >> (8 * jj) & 0xFFu);
            int o1 = col[0], o2 = 0, o3 = 0, o4 = 0;          // the old values of the nodes n - 1 .. n - 4
            col[0] = (q * 4 + jj + 1) * ins;
            // (the structure words are made opaque per character step: what is derived from them is then worked out on the scalar unit
            // where it is used, not kept in a hundred scalar registers across the loop and spilled)
            uint32_t s0 = S0, s1 = S1;
            asm volatile("" : "+s"(s0), "+s"(s1));
#pragma unroll
            for (int n = 1; n <= MC; ++n) {
                const uint32_t fld = (n <= 16 ? s0 : s1) >> (2 * ((n - 1) & 15)) & 3u;          // jl - 1
                const int      old = col[n];
                int            best = old + ins;
                if (fld == 0) LM_EDGE(1, o1, 0, del)
                else {
                    LM_EDGE(1, o1, split, dsp)
                    if (n >= 2) {
                        if (fld == 1) LM_EDGE(2, o2, 0, del)
                        else {
                            LM_EDGE(2, o2, split, dsp)
                            if (n >= 3) {
                                if (fld == 2) LM_EDGE(3, o3, 0, del)
                                else {
                                    LM_EDGE(3, o3, split, dsp)
                                    if (n >= 4) LM_EDGE(4, o4, 0, del)
                                }
                            }
                        }
                    }
                }
                col[n] = best;
                o4 = o3; o3 = o2; o2 = o1; o1 = old;
            }
        }
    }
    int res = col[0];
#pragma unroll
    for (int n = 1; n <= MC; ++n) res = n == N ? col[n] : res;
    return res;
}
#undef LM_EDGE

// ---- a wave a word: the free segmentation, the table of one entry and its backtrack -------------------------------------------------
// what one lane writes another lane of the same wave reads: the wave runs in lockstep and its LDS operations complete in order
__device__ __forceinline__ void lm_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int lm_wave_min(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}

// the minimum of a cost row, on every lane
__device__ __forceinline__ int lm_row_min(const uint8_t *row, int lane)
{
    return lm_wave_min(min((int)row[lane], (int)row[64]));
}

// the LDS of one wave: lane j holds the column j of the table, the table and the byte every (node, edge, character) read cost are kept
// here, and lane 0 walks back through them
struct LmWaveLds {
    int32_t T[(LM_MAX_NODES + 1) * LM_TROW];
    uint8_t cc[LM_MAX_NODES + 1][4][LM_TROW + 3];          // the byte SUB(i) into node n reads for the character j
    int32_t node_run[LM_MAX_NODES + 1], node_fp[LM_MAX_NODES + 1];
    uint8_t node_ja[LM_MAX_NODES + 1];                     // the node's local index j | its run's atoms << 4
    int32_t part_run[LM_MAX_NODES], part_piece[LM_MAX_NODES];
    uint8_t from[32];
    int32_t rec[4];                                        // n_parts, n_del, n_ins
};

// The m runs from `first` on, one after the other: the free segmentation of each on the minima of its rows (returned: the word's
// str_er_word_split cost), and the nodes into L while they are at most 32.  N: the word's nodes, LM_MAX_NODES + 1 for more.
__device__ __forceinline__ int32_t lm_wave_nodes(LmWaveLds &L, const str_er_run_split *__restrict__ splits, const uint8_t *__restrict__ run_costs,
                                                 const uint8_t *__restrict__ piece_costs, int first, int m, int split, int lane, int &N)
{
    int32_t fc = 0;
    N = 0;
    for (int t = 0; t < m; ++t) {
        const int      r = first + t, A = __builtin_amdgcn_readfirstlane(lm_atoms(splits, r)), fp = __builtin_amdgcn_readfirstlane(splits[r].first_piece);
        const uint8_t *rrow = run_costs + (size_t)r * WM_ALPHABET;
        int            D[5];
        D[0] = 0;
#pragma unroll
        for (int j = 1; j <= 4; ++j) {
            D[j] = 0;
            if (j <= A) {
                int best = 0x7FFFFFFF;
#pragma unroll
                for (int i = 0; i < j; ++i) {
                    const int k = lm_piece_index(A, i, j);
                    const int v = D[i] + lm_row_min(k < 0 ? rrow : piece_costs + ((size_t)fp + (size_t)k) * WM_ALPHABET, lane) + (i > 0 ? split : 0);
                    best = min(best, v);
                }
                D[j] = best;
                if (lane == 0 && N + j <= LM_MAX_NODES) { L.node_run[N + j] = r; L.node_fp[N + j] = fp; L.node_ja[N + j] = (uint8_t)(j | A << 4); }
            }
        }
        int da = D[1];
#pragma unroll
        for (int j = 2; j <= 4; ++j) da = j == A ? D[j] : da;
        fc += da;
        N = min(N + A, LM_MAX_NODES + 1);
    }
    return fc;
}

// The table of a string of `len` labels over the N <= 32 nodes lm_wave_nodes left in L, a column a lane (the lane j = min(lane, 32) brings
// the label j of the string in a, 1 .. len, and its case partner -- or a again -- in ap), and lane 0's backtrack: L.rec, L.from and L.part_*
// as lm_wave_store writes them out.  run (uniform) false: the record of a word without a string.  L.T[N * LM_TROW + len] is the cost; the
// caller's lm_wave_sync comes before he reads L.
__device__ __forceinline__ void lm_wave_path(LmWaveLds &L, const WmParams &prm, int split, const uint8_t *__restrict__ run_costs,
                                             const uint8_t *__restrict__ piece_costs, int a, int ap, int len, int N, bool run, int lane)
{
    if (lane == 0) { L.rec[0] = L.rec[1] = L.rec[2] = 0; }
    if (lane < 32) L.from[lane] = 0xFF;
    if (run) {          // (uniform) the table, a column a lane, and the backtrack
        const int j = min(lane, 32);
        int32_t  *Tw = L.T;
        if (lane <= 32) Tw[j] = j * prm.ins;
        lm_wave_sync();
        for (int n = 1; n <= N; ++n) {
            const int      r = L.node_run[n], fp = L.node_fp[n], jl = L.node_ja[n] & 15, A = L.node_ja[n] >> 4;
            const uint8_t *rrow = run_costs + (size_t)r * WM_ALPHABET;
            int            X = 0x3FFFFFFF;
            for (int i = 0; i < jl; ++i) {
                const int      f = n - jl + i, k = lm_piece_index(A, i, jl), s = i > 0 ? split : 0;
                const uint8_t *row = k < 0 ? rrow : piece_costs + ((size_t)fp + (size_t)k) * WM_ALPHABET;
                const int      c = min((int)row[a], (int)row[ap]);
                if (lane <= 32) L.cc[n][i][j] = (uint8_t)c;
                if (j >= 1) X = min(X, Tw[f * LM_TROW + j - 1] + c + s);
                X = min(X, Tw[f * LM_TROW + j] + prm.del + s);
            }
            int v = X - j * prm.ins;          // the INS chain: a prefix minimum over the lanes
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_up(v, off, 64);
                if (lane >= off) v = min(v, o);
            }
            if (lane <= 32) Tw[n * LM_TROW + j] = v + j * prm.ins;
            lm_wave_sync();
        }
        if (lane == 0) {          // the first candidate, in the contract's order, that attains the cell
            int n = N, jj = len, np = 0, nd = 0, ni = 0;
            while (n > 0 || jj > 0) {          // (every step lowers n or jj; a part is taken only while n > 0, so np stays below N <= 32)
                const int d = Tw[n * LM_TROW + jj];
                int       mv = -1, jl = 0;
                if (n > 0) {
                    jl = L.node_ja[n] & 15;
                    for (int i = 0; i < jl && mv < 0; ++i) {
                        const int f = n - jl + i, s = i > 0 ? split : 0;
                        if (jj >= 1 && Tw[f * LM_TROW + jj - 1] + (int)L.cc[n][i][jj] + s == d) mv = 2 * i;
                        else if (Tw[f * LM_TROW + jj] + prm.del + s == d) mv = 2 * i + 1;
                    }
                }
                if (mv < 0) {          // INS: the character jj is inserted at the node n
                    if (jj <= 0) break;
                    L.from[jj - 1] = (uint8_t)(np | 0x80);
                    ++ni; --jj;
                    continue;
                }
                const int i = mv >> 1, A = L.node_ja[n] >> 4, k = lm_piece_index(A, i, jl);
                L.part_run[np] = L.node_run[n]; L.part_piece[np] = k < 0 ? -1 : L.node_fp[n] + k;
                if (mv & 1) ++nd;
                else { L.from[jj - 1] = (uint8_t)np; --jj; }
                ++np;
                n -= jl - i;
            }
            L.rec[0] = np; L.rec[1] = nd; L.rec[2] = ni;
        }
    }
}

// lm_wave_path for the entry `entry` of the lexicon.  run (uniform) false: the record of a word without an entry.  Returns the entry's
// length (0 without).
__device__ __forceinline__ int lm_wave_winner(LmWaveLds &L, const WmLexDev &lex, const WmParams &prm, int split, const uint8_t *__restrict__ run_costs,
                                              const uint8_t *__restrict__ piece_costs, int entry, int N, bool run, int lane)
{
    int len = 0, a = 0;          // a: the character j of the entry (1 .. len)
    if (run) {          // (uniform)
        const int pos = __builtin_amdgcn_readfirstlane(lex.pos[entry]), g = pos >> 6, el = pos & 63;
        len = 1;
        while (len < 32 && g >= lex.len_first[len + 1]) ++len;
        const int j = min(lane, 32);
        if (j >= 1 && j <= len) a = (int)(lex.chars[lex.goff[g] + (size_t)((j - 1) >> 2) * WM_GROUP + el] >> (8 * ((j - 1) & 3)) & 0xFFu);
    }
    lm_wave_path(L, prm, split, run_costs, piece_costs, a, lex.fold ? wm_partner(a) : a, len, N, run, lane);
    return len;
}

// lm_wave_path for the l labels at s (l <= 32, read as they are: no fold); run (uniform) false: no string
__device__ __forceinline__ void lm_wave_labels(LmWaveLds &L, const WmParams &prm, int split, const uint8_t *__restrict__ run_costs,
                                               const uint8_t *__restrict__ piece_costs, const uint8_t *__restrict__ s, int l, int N, bool run, int lane)
{
    const int j = min(lane, 32);
    int       a = 0;
    if (run && j >= 1 && j <= l) a = (int)s[j - 1];
    lm_wave_path(L, prm, split, run_costs, piece_costs, a, a, l, N, run, lane);
}

// after the caller's lm_wave_sync: the 32 source bytes to src and the L.rec[0] parts, in word order, to parts (pairs of int32)
__device__ __forceinline__ void lm_wave_store(const LmWaveLds &L, int len, int lane, uint8_t *__restrict__ src, int32_t *__restrict__ parts)
{
    const int np = L.rec[0];
    if (lane < 32) {          // a read character: its part in word order; an inserted one: the parts that end at or before its node
        const int fb = L.from[lane];
        src[lane] = lane < len ? (fb & 0x80 ? (uint8_t)(0x80 | (np - (fb & 0x7F))) : (uint8_t)(np - 1 - fb)) : (uint8_t)0xFF;
    }
    if (lane < np) {          // (n_parts <= N <= 32, the slots of the word)
        parts[2 * (size_t)lane] = L.part_run[np - 1 - lane];
        parts[2 * (size_t)lane + 1] = L.part_piece[np - 1 - lane];
    }
}

} // namespace

} // namespace str_er
