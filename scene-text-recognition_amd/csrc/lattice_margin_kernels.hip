// lattice_margin_kernels.hip -- the margins of the lattice decoder on the device (gfx950): k_lattice_margin makes the min-marginals of
// the recurrence of k_lattice_decode -- for every edge of a word's lattice and every reading of it the cost of the cheapest whole path
// that takes the edge and reads it that way -- and from them the reading margin and the cut margin of every part of the decoded path
// and of the word.  Integers only and no atomics: the output is the same bytes every time.  The rules are stated for the host in
// lattice_margin_rules.h; the contract is at str_er_lattice_margin in str_er.h.
//
// A word per wave, LM_WORDS words per workgroup, behind k_lattice_decode, whose record, labels, sources and parts say which edges the
// decoded path takes and how it reads them.  The table is staged as in k_word_margin: rows of 17 words, so that the backward product
// reads a row per lane from an odd stride (no two lanes on one bank) against a vector every lane reads at one address (a broadcast);
// the row helpers are that kernel's, stated again here because its file stays as it is.  The states 64 and 65 live in the second
// register of the lanes 0 and 1.
//
// Forward: the pass of k_lattice_decode without back pointers.  Per node f the wave keeps V_f and P_f[b] = min_a (V_f[a] + B[a][b]) in
// LDS, not S per edge: S_e = P_f + C_e + s.  Every finite forward value is the cost of a path of at most 32 edges, and an edge adds at
// most B + C + SPLIT = 765 read (or DEL + SPLIT = 510 dropped) and B + INS = 510 for a character inserted behind it: at most
// 32 * 5 * 255 = 40800, and P at most 255 more, 41055 < 65535.  So 16 bits hold them and 0xFFFF stands for INF: a value that is not
// below INF is a sum with some V_0[a] = INF in it, it never wins against a finite one and is reported as -1 whatever was added to it.
// The backward values stay in 32-bit registers.
//
// Backward, over the nodes n = N .. 1: GU_n (one transposed product if INS is on), then for every edge (i, j) into n its 66 marginals
// from P and V of its source node, its minimum m_e (to a small LDS array) and, if the decoded path takes it, the part's reading margin;
// and the edge's row and GU_n are min-ed into H and the DEL term of the source's local node -- min-plus distributes, so a node needs
// one transposed product over H, not one per edge.  H and the DEL term of the up to four open local nodes of the run are named
// registers picked by compile-time indices in the unrolled loop over i, the mirror of the forward ring.  Which in-edge of a node is on
// the path, and its part, is scattered into LDS from the decoder's parts before the pass; the end node of part k is a prefix sum of the
// parts' atoms over the lanes.  After the pass lane k forms part k's cut margin from at most nine entries of m_e.  The record is made
// from wave minima over margin << 5 | part; every per-part output leaves in one store of 32 lanes.  The loops over the nodes are
// run-time loops and no array lives in registers.
//
// LDS per workgroup: 4488 (table) + 2 * 1088 (vectors) + 2 * 16896 (V and P) + 2048 (m_e) + 640 (the nodes' runs) + 384 (the path) =
// 43536 bytes with the padding between them: three workgroups (twelve waves) a CU by LDS.
#include <hip/hip_runtime.h>

#include "lattice_margin_kernels.h"
#include "word_decode_device.h"

namespace str_er {

namespace {

constexpr int      LM_THREADS = 64 * LM_WORDS, LM_MAX_NODES = 32, LM_ROW_WORDS = WD_ROW / 4;
constexpr uint32_t LM_NONE16 = 0xFFFFu, LM_OPEN = 4u * WD_INF;          // LM_OPEN: nothing min-ed in yet

static_assert(LM_PARTS == LM_MAX_NODES && LM_READINGS == WD_STATES && LM_FROM == 4, "the layout of the contract");

__device__ __forceinline__ uint32_t lm_load16(uint16_t v) { return v == LM_NONE16 ? WD_INF : (uint32_t)v; }
__device__ __forceinline__ uint16_t lm_store16(uint32_t v) { return (uint16_t)min(v, LM_NONE16); }

__device__ __forceinline__ int lm_wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the piece (i, j) of a run of A atoms in the order by (i, j) without (0, A); -1: the run itself
__device__ __forceinline__ int lm_piece_index(int A, int i, int j)
{
    if (i == 0) return j == A ? -1 : j - 1;
    return (A - 1) + (i - 1) * A - (i - 1) * i / 2 + (j - i - 1);
}

__device__ __forceinline__ int lm_atoms(const str_er_run_split *splits, int r) { return min(max(splits[r].n_cuts, 0), 3) + 1; }

// min over c in [0, 65) of B[lane][c] + vec[c]; brow = the words of the table's row of the lane.  Fully unrolled: every offset is an immediate.
__device__ __forceinline__ uint32_t lm_product_t(const uint32_t *vec, const uint32_t *brow)
{
    uint32_t best = ~0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t b4 = brow[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) best = min(best, vec[4 * k + j] + ((b4 >> (8 * j)) & 255u));
    }
    return min(best, vec[64] + (brow[16] & 255u));
}

// the same for the row a = 64 or 65 of the table, turned round: a lane a column, the column 64 in lane 0; every lane gets the minimum
__device__ __forceinline__ uint32_t lm_row(const uint8_t *Bs, int lane, int a, uint32_t v_lo, uint32_t v_64)
{
    uint32_t t = v_lo + (uint32_t)Bs[a * WD_ROW + lane];
    if (lane == 0) t = min(t, v_64 + (uint32_t)Bs[a * WD_ROW + 64]);
    return wd_wave_min(t);
}

// forward: one edge into the node under construction, from a local node with the products pv (targets 0 .. 63) and qv (target 64)
// and the values v_lo / v_hi of V there
__device__ __forceinline__ void lm_fwd_edge(int lane, uint32_t pv, uint32_t qv, uint32_t v_lo, uint32_t v_hi, uint32_t cb, uint32_t c64, uint32_t s, uint32_t del,
                                            uint32_t &u_lo, uint32_t &u_hi)
{
    u_lo = min(u_lo, pv + cb + s);
    if (lane == 0) u_hi = min(u_hi, qv + c64 + s);
    if (del > 0) {
        u_lo = min(u_lo, v_lo + del + s);
        u_hi = min(u_hi, v_hi + del + s);
    }
}

// what the backward pass knows of the edge it is at
struct LmEdge {
    uint32_t m_lo, m_64, m_65;          // the marginals: the lane's label, 64 (lane 0), dropped (every lane; INF where it was not made)
    uint32_t least;                     // m_e
};

// backward: one edge into node n from the local node whose H and DEL term are h_* and d_*: its marginals, and its row and GU_n min-ed in
__device__ __forceinline__ LmEdge lm_bwd_edge(int lane, const uint16_t *sPf, const uint16_t *sVf, uint32_t cb, uint32_t c64, uint32_t s, uint32_t del, uint32_t gu_lo,
                                              uint32_t gu_hi, bool want_65, uint32_t &h_lo, uint32_t &h_64, uint32_t &d_lo, uint32_t &d_hi)
{
    LmEdge e;
    e.m_lo = lm_load16(sPf[lane]) + cb + s + gu_lo;
    e.m_64 = lm_load16(sPf[64]) + c64 + s + gu_hi;          // (counts in lane 0 alone)
    uint32_t t = WD_INF;
    if (del > 0) {
        t = lm_load16(sVf[lane]) + del + s + gu_lo;
        if (lane < 2) t = min(t, lm_load16(sVf[64 + lane]) + del + s + gu_hi);
        d_lo = min(d_lo, gu_lo);
        d_hi = min(d_hi, gu_hi);
    }
    uint32_t all = min(e.m_lo, t);
    if (lane == 0) all = min(all, e.m_64);
    e.least = wd_wave_min(all);
    e.m_65 = want_65 ? wd_wave_min(t) : WD_INF;
    h_lo = min(h_lo, cb + gu_lo);
    h_64 = min(h_64, c64 + gu_hi);
    return e;
}

__global__ void __launch_bounds__(LM_THREADS)
k_lattice_margin(const uint8_t *__restrict__ bigram, int ins, int del, int split, const str_er_run_split *__restrict__ splits, const uint8_t *__restrict__ run_costs,
                 const uint8_t *__restrict__ piece_costs, const int32_t *__restrict__ first_run, const int32_t *__restrict__ n_of, const int32_t *__restrict__ slot,
                 int n_words, const int32_t *__restrict__ dec, const uint8_t *__restrict__ chars, const uint8_t *__restrict__ src, const int32_t *__restrict__ parts,
                 int32_t *__restrict__ margins, int32_t *__restrict__ read_margin, int32_t *__restrict__ cut_margin, uint8_t *__restrict__ read,
                 uint8_t *__restrict__ alt, uint8_t *__restrict__ cut_alt, int32_t *__restrict__ edge_min, int32_t *__restrict__ marginals)
{
    __shared__ __attribute__((aligned(16))) uint32_t Bw[WD_STATES * LM_ROW_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t vk[LM_WORDS][WD_ROW], uk[LM_WORDS][WD_ROW];
    __shared__ uint16_t sV[LM_WORDS][LM_MAX_NODES][WD_STATES], sP[LM_WORDS][LM_MAX_NODES][WD_STATES];
    __shared__ int32_t  em[LM_WORDS][LM_MAX_NODES][LM_FROM];
    __shared__ int32_t  node_run[LM_WORDS][LM_MAX_NODES];
    __shared__ uint8_t  node_ja[LM_WORDS][LM_MAX_NODES];          // the node's local index j | its run's atoms << 4
    __shared__ uint8_t  xr[LM_WORDS][LM_PARTS], pin[LM_WORDS][LM_MAX_NODES], pk[LM_WORDS][LM_MAX_NODES];
    uint8_t  *Bs = reinterpret_cast<uint8_t *>(Bw);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t = tid; t < WD_STATES * WD_ROW; t += LM_THREADS) {
        const int a = t / WD_ROW, b = t - a * WD_ROW;
        Bs[t] = b < WD_STATES ? bigram[a * WD_STATES + b] : (uint8_t)0;
    }
    __syncthreads();          // (the only barrier of the workgroup: from here on a wave is on its own)
    const int w = (int)blockIdx.x * LM_WORDS + wave;
    if (w >= n_words) return;
    const int    first = __builtin_amdgcn_readfirstlane(first_run[w]), m = max(0, __builtin_amdgcn_readfirstlane(n_of[w]));
    const size_t base = (size_t)__builtin_amdgcn_readfirstlane(slot[w]);
    int          N = 0, n_edges = 0;
    for (int t = 0; t < m; t += 64) {
        const int A = t + lane < m ? lm_atoms(splits, first + t + lane) : 0;
        N += lm_wave_sum(A);
        n_edges += lm_wave_sum(A * (A + 1) / 2);
    }
    N = __builtin_amdgcn_readfirstlane(N);
    n_edges = __builtin_amdgcn_readfirstlane(n_edges);
    const int  n_chars = __builtin_amdgcn_readfirstlane(dec[(size_t)w * 8 + 2]), n_parts = __builtin_amdgcn_readfirstlane(dec[(size_t)w * 8 + 7]);
    const bool ok = N >= 1 && N <= LM_MAX_NODES && n_parts >= 1 && n_parts <= N && n_chars >= 0 && n_chars <= 64;
    int32_t    my_rm = -1, my_cm = -1;                      // of part `lane`, for lane < n_parts
    uint32_t   my_rd = 0xFFu, my_alt = 0xFFu, my_ca = 0xFFu;
    int32_t   *mg = marginals ? marginals + (size_t)w * (LM_MAX_NODES * LM_FROM * LM_READINGS) : nullptr;
    if (ok) {
        uint32_t       *vkw = vk[wave], *ukw = uk[wave];
        const uint8_t  *bcol = Bs + lane;
        const uint32_t *brow = Bw + lane * LM_ROW_WORDS;
        const uint32_t  sp = (uint32_t)split, dl = (uint32_t)max(del, 0);
        // the decoded path: the reading of every part, and per node the in-edge the path takes and its part
        if (lane < LM_MAX_NODES) {
            xr[wave][lane] = (uint8_t)WD_E; pin[wave][lane] = 0xFF; pk[wave][lane] = 0xFF;
#pragma unroll
            for (int i = 0; i < LM_FROM; ++i) em[wave][lane][i] = -1;
        }
        wd_wave_sync();
        if (lane < n_chars) {
            const uint32_t from = src[(size_t)w * 64 + lane];
            if (from < (uint32_t)n_parts) xr[wave][from] = chars[(size_t)w * 64 + lane];          // (bit 7 set: inserted, no part)
        }
        int my_n = 0, my_i = 0, my_j = 1, my_A = 1;          // part `lane`: the node it ends at, its edge and its run's atoms
        if (lane < n_parts) {
            const int run = parts[2 * (base + (size_t)lane)], piece = parts[2 * (base + (size_t)lane) + 1];
            if (run >= first && run < first + m) {
                my_A = lm_atoms(splits, run);
                const int kk = piece < 0 ? -1 : piece - splits[run].first_piece;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = i + 1; j <= 4; ++j)
                        if (j <= my_A && lm_piece_index(my_A, i, j) == kk) { my_i = i; my_j = j; }
            }
            my_n = my_j - my_i;
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {          // the parts' atoms summed over the lanes up to and with this one
            const int v = __shfl_up(my_n, off, 64);
            if (lane >= off) my_n += v;
        }
        const bool my_ok = lane < n_parts && my_n >= my_j && my_n <= N;
        if (my_ok) { pin[wave][my_n - 1] = (uint8_t)my_i; pk[wave][my_n - 1] = (uint8_t)lane; }
        // the forward pass of k_lattice_decode: V_0 is the boundary at 0, every character at INF
        uint32_t key_lo = WD_INF << 7 | (uint32_t)lane;
        uint32_t key_hi = lane == 1 ? (uint32_t)WD_E : WD_INF << 7 | (uint32_t)(64 + (lane & 1));
        vkw[lane] = key_lo;
        if (lane < 2) vkw[64 + lane] = key_hi;
        {
            // the ring: the products and the values of the local nodes 0 .. 3 of the current run
            uint32_t p0 = 0, p1 = 0, p2 = 0, p3 = 0, q0 = 0, q1 = 0, q2 = 0, q3 = 0;
            uint32_t vl0 = 0, vl1 = 0, vl2 = 0, vl3 = 0, vh0 = 0, vh1 = 0, vh2 = 0, vh3 = 0;
            int            r = first - 1, A = 0, j = 0, fp = 0;
            const uint8_t *rrow = run_costs;
            for (int n = 1; n <= N; ++n) {
                wd_wave_sync();
                {          // the product of the node n - 1, final by now
                    const uint32_t p = wd_product<WD_STATES>(vkw, key_lo, key_hi, bcol) >> 7, q = wd_column(Bs, lane, 64, key_lo, key_hi, 2) >> 7;
                    const uint32_t v_lo = key_lo >> 7, v_hi = key_hi >> 7;
                    sV[wave][n - 1][lane] = lm_store16(v_lo); sP[wave][n - 1][lane] = lm_store16(p);
                    if (lane < 2) sV[wave][n - 1][64 + lane] = lm_store16(v_hi);
                    if (lane == 0) sP[wave][n - 1][64] = lm_store16(q);
                    if (j == A) {
                        ++r;
                        A = __builtin_amdgcn_readfirstlane(lm_atoms(splits, r)); fp = __builtin_amdgcn_readfirstlane(splits[r].first_piece);
                        rrow = run_costs + (size_t)r * WD_ALPHABET;
                        j = 0;
                        p0 = p; q0 = q; vl0 = v_lo; vh0 = v_hi;
                    } else if (j == 1) { p1 = p; q1 = q; vl1 = v_lo; vh1 = v_hi; }
                    else if (j == 2) { p2 = p; q2 = q; vl2 = v_lo; vh2 = v_hi; }
                    else { p3 = p; q3 = q; vl3 = v_lo; vh3 = v_hi; }
                }
                ++j;
                uint32_t u_lo = WD_INF, u_hi = WD_INF;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < j) {
                        const int      k = lm_piece_index(A, i, j);
                        const uint8_t *row = k < 0 ? rrow : piece_costs + ((size_t)fp + (size_t)k) * WD_ALPHABET;
                        const uint32_t cb = row[lane], c64 = row[64], s = i > 0 ? sp : 0u;
                        if (i == 0) lm_fwd_edge(lane, p0, q0, vl0, vh0, cb, c64, s, dl, u_lo, u_hi);
                        else if (i == 1) lm_fwd_edge(lane, p1, q1, vl1, vh1, cb, c64, s, dl, u_lo, u_hi);
                        else if (i == 2) lm_fwd_edge(lane, p2, q2, vl2, vh2, cb, c64, s, dl, u_lo, u_hi);
                        else lm_fwd_edge(lane, p3, q3, vl3, vh3, cb, c64, s, dl, u_lo, u_hi);
                    }
                uint32_t w_lo = u_lo, w_hi = u_hi;
                if (ins > 0) {
                    const uint32_t uk_lo = u_lo << 7 | (uint32_t)lane, uk_hi = u_hi << 7 | 64u;          // (uk_hi counts in lane 0 alone)
                    ukw[lane] = uk_lo;
                    if (lane == 0) ukw[64] = uk_hi;
                    wd_wave_sync();
                    const uint32_t i_lo = wd_product<WD_ALPHABET>(ukw, uk_lo, uk_hi, bcol);
                    const uint32_t i_64 = wd_column(Bs, lane, 64, uk_lo, uk_hi, 1);
                    w_lo = min(u_lo, (i_lo >> 7) + (uint32_t)ins);
                    if (lane == 0) w_hi = min(u_hi, (i_64 >> 7) + (uint32_t)ins);
                }
                key_lo = w_lo << 7 | (uint32_t)lane;
                key_hi = w_hi << 7 | (uint32_t)(64 + (lane & 1));
                vkw[lane] = key_lo;
                if (lane < 2) vkw[64 + lane] = key_hi;
                if (lane == 0) { node_run[wave][n - 1] = r; node_ja[wave][n - 1] = (uint8_t)(j | A << 4); }
            }
        }
        const uint32_t cost = wd_column(Bs, lane, WD_E, key_lo, key_hi, 2) >> 7;
        wd_wave_sync();
        // the backward pass: G_N[a] = B[a][E]; G of the states 64 and 65 in g_hi of the lanes 0 and 1
        uint32_t g_lo = Bs[lane * WD_ROW + WD_E], g_hi = lane < 2 ? (uint32_t)Bs[(64 + lane) * WD_ROW + WD_E] : WD_INF;
        // the ring: H (h*l: the labels 0 .. 63, h*h: 64 in lane 0) and the DEL term (d*l, d*h: 64 and 65 in the lanes 0 and 1) of the local nodes 0 .. 3
        uint32_t h0l = LM_OPEN, h1l = LM_OPEN, h2l = LM_OPEN, h3l = LM_OPEN, h0h = LM_OPEN, h1h = LM_OPEN, h2h = LM_OPEN, h3h = LM_OPEN;
        uint32_t d0l = LM_OPEN, d1l = LM_OPEN, d2l = LM_OPEN, d3l = LM_OPEN, d0h = LM_OPEN, d1h = LM_OPEN, d2h = LM_OPEN, d3h = LM_OPEN;
        for (int n = N; n >= 1; --n) {
            const int      ja = __builtin_amdgcn_readfirstlane((int)node_ja[wave][n - 1]), j = ja & 15, A = ja >> 4;
            const int      r = __builtin_amdgcn_readfirstlane(node_run[wave][n - 1]), fp = __builtin_amdgcn_readfirstlane(splits[r].first_piece);
            const int      on = __builtin_amdgcn_readfirstlane((int)pin[wave][n - 1]), k_on = __builtin_amdgcn_readfirstlane((int)pk[wave][n - 1]);
            const uint32_t x = on < LM_FROM && k_on < LM_PARTS ? (uint32_t)xr[wave][k_on] : 0xFFu;
            const uint8_t *rrow = run_costs + (size_t)r * WD_ALPHABET;
            if (j == A) {          // the last node of its run: nothing leaves the run's local nodes yet
                h0l = h1l = h2l = h3l = h0h = h1h = h2h = h3h = LM_OPEN;
                d0l = d1l = d2l = d3l = d0h = d1h = d2h = d3h = LM_OPEN;
            }
            // GU: a character inserted behind the edge's
            uint32_t gu_lo = g_lo, gu_hi = g_hi;
            if (ins > 0) {
                wd_wave_sync();
                vkw[lane] = g_lo;
                if (lane == 0) vkw[64] = g_hi;
                wd_wave_sync();
                const uint32_t t_lo = lm_product_t(vkw, brow), t_64 = lm_row(Bs, lane, 64, g_lo, g_hi);
                gu_lo = min(g_lo, t_lo + (uint32_t)ins);
                if (lane == 0) gu_hi = min(g_hi, t_64 + (uint32_t)ins);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < j) {
                    const int       k = lm_piece_index(A, i, j), f = n - j + i;
                    const uint8_t  *row = k < 0 ? rrow : piece_costs + ((size_t)fp + (size_t)k) * WD_ALPHABET;
                    const uint32_t  cb = row[lane], c64 = row[64], s = i > 0 ? sp : 0u;
                    const uint16_t *sPf = sP[wave][f], *sVf = sV[wave][f];
                    const bool      want_65 = dl > 0 && (mg != nullptr || on == i);
                    LmEdge          e;
                    if (i == 0) e = lm_bwd_edge(lane, sPf, sVf, cb, c64, s, dl, gu_lo, gu_hi, want_65, h0l, h0h, d0l, d0h);
                    else if (i == 1) e = lm_bwd_edge(lane, sPf, sVf, cb, c64, s, dl, gu_lo, gu_hi, want_65, h1l, h1h, d1l, d1h);
                    else if (i == 2) e = lm_bwd_edge(lane, sPf, sVf, cb, c64, s, dl, gu_lo, gu_hi, want_65, h2l, h2h, d2l, d2h);
                    else e = lm_bwd_edge(lane, sPf, sVf, cb, c64, s, dl, gu_lo, gu_hi, want_65, h3l, h3h, d3l, d3h);
                    if (lane == 0) em[wave][n - 1][i] = e.least < WD_INF ? (int32_t)e.least : -1;
                    if (on == i) {          // the edge is part k_on of the path: the wave minimum of marginal << 7 | reading, the decoded reading left out
                        uint32_t key = (uint32_t)lane != x && e.m_lo < WD_INF ? e.m_lo << 7 | (uint32_t)lane : ~0u;
                        if (lane == 0 && x != 64u && e.m_64 < WD_INF) key = min(key, e.m_64 << 7 | 64u);
                        if (lane == 1 && x != 65u && e.m_65 < WD_INF) key = min(key, e.m_65 << 7 | 65u);
                        key = wd_wave_min(key);
                        if (lane == k_on) { my_rm = (int32_t)(key >> 7) - (int32_t)cost; my_rd = x; my_alt = key & 127u; }
                    }
                    if (mg) {
                        int32_t *out = mg + ((n - 1) * LM_FROM + i) * LM_READINGS;
                        out[lane] = e.m_lo < WD_INF ? (int32_t)e.m_lo : -1;
                        if (lane == 0) out[64] = e.m_64 < WD_INF ? (int32_t)e.m_64 : -1;
                        if (lane == 1) out[65] = e.m_65 < WD_INF ? (int32_t)e.m_65 : -1;
                    }
                }
            // G of the node before, the local node j - 1 of this run: every edge that leaves it has been seen
            uint32_t h_lo, h_64, d_lo, d_hi;
            if (j == 1) { h_lo = h0l; h_64 = h0h; d_lo = d0l; d_hi = d0h; }
            else if (j == 2) { h_lo = h1l; h_64 = h1h; d_lo = d1l; d_hi = d1h; }
            else if (j == 3) { h_lo = h2l; h_64 = h2h; d_lo = d2l; d_hi = d2h; }
            else { h_lo = h3l; h_64 = h3h; d_lo = d3l; d_hi = d3h; }
            const uint32_t s = j > 1 ? sp : 0u;
            wd_wave_sync();
            ukw[lane] = h_lo;
            if (lane == 0) ukw[64] = h_64;
            wd_wave_sync();
            const uint32_t n_lo = lm_product_t(ukw, brow), n_64 = lm_row(Bs, lane, 64, h_lo, h_64), n_65 = lm_row(Bs, lane, WD_E, h_lo, h_64);
            g_lo = n_lo + s;
            g_hi = lane == 0 ? n_64 + s : lane == 1 ? n_65 + s : WD_INF;
            if (dl > 0) {
                g_lo = min(g_lo, dl + s + d_lo);
                if (lane < 2) g_hi = min(g_hi, dl + s + d_hi);
            }
        }
        wd_wave_sync();
        // the cut margin of part `lane`: the other edges of its run over its atoms, in the order of (i', j')
        if (my_ok) {
            const int off = my_n - my_j;
            uint32_t  best = ~0u;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = i + 1; j <= 4; ++j)
                    if (j <= my_A && i < my_j && j > my_i && !(i == my_i && j == my_j) && off + j <= N) {
                        const int32_t v = em[wave][off + j - 1][i];
                        if (v >= 0 && (uint32_t)v < best) { best = (uint32_t)v; my_ca = (uint32_t)(i | j << 4); }
                    }
            if (best != ~0u) my_cm = (int32_t)best - (int32_t)cost;
        }
    }
    // the word: the smallest margins at the smallest part (a margin is below 2^16)
    const bool     mine = ok && lane < n_parts && my_rm >= 0;
    const uint32_t rkey = wd_wave_min(mine ? (uint32_t)my_rm << 5 | (uint32_t)lane : ~0u);
    const uint32_t ckey = wd_wave_min(mine && my_cm >= 0 ? (uint32_t)my_cm << 5 | (uint32_t)lane : ~0u);
    const int      rpart = rkey != ~0u ? (int)(rkey & 31u) : 0, cpart = ckey != ~0u ? (int)(ckey & 31u) : 0;
    const int32_t  rread = __shfl((int)my_rd, rpart, 64), ralt = __shfl((int)my_alt, rpart, 64), cca = __shfl((int)my_ca, cpart, 64);
    if (lane < 8) {
        int32_t v;
        if (lane < 4) v = rkey == ~0u ? -1 : lane == 0 ? (int32_t)(rkey >> 5) : lane == 1 ? rpart : lane == 2 ? rread : ralt;
        else if (lane < 7) v = ckey == ~0u || rkey == ~0u ? -1 : lane == 4 ? (int32_t)(ckey >> 5) : lane == 5 ? cpart : cca;
        else v = rkey == ~0u ? 0 : n_edges;
        margins[(size_t)w * 8 + lane] = v;
    }
    if (lane < LM_PARTS) {
        read_margin[(size_t)w * LM_PARTS + lane] = my_rm;
        cut_margin[(size_t)w * LM_PARTS + lane] = my_cm;
        read[(size_t)w * LM_PARTS + lane] = (uint8_t)my_rd;
        alt[(size_t)w * LM_PARTS + lane] = (uint8_t)my_alt;
        cut_alt[(size_t)w * LM_PARTS + lane] = (uint8_t)my_ca;
    }
    if (edge_min)
        for (int t = lane; t < LM_MAX_NODES * LM_FROM; t += 64) edge_min[(size_t)w * (LM_MAX_NODES * LM_FROM) + t] = ok ? em[wave][t >> 2][t & 3] : -1;
    if (mg)          // -1 where there is no edge (an edge's marginals are written, once each, in the pass)
        for (int t = 0; t < LM_MAX_NODES * LM_FROM; ++t) {
            const int32_t v = ok ? em[wave][t >> 2][t & 3] : -1;
            if (v < 0) {
                mg[t * LM_READINGS + lane] = -1;
                if (lane < 2) mg[t * LM_READINGS + 64 + lane] = -1;
            }
        }
}

} // namespace

void launch_lattice_margin(hipStream_t s, const uint8_t *bigram, int ins, int del, int split, const str_er_run_split *splits, const uint8_t *run_costs,
                           const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of, const int32_t *slot, int n_words, const int32_t *dec,
                           const uint8_t *chars, const uint8_t *src, const int32_t *parts, void *margins, int32_t *read_margin, int32_t *cut_margin, uint8_t *read,
                           uint8_t *alt, uint8_t *cut_alt, int32_t *edge_min, int32_t *marginals)
{
    if (n_words <= 0) return;
    hipLaunchKernelGGL(k_lattice_margin, dim3((unsigned)((n_words + LM_WORDS - 1) / LM_WORDS)), dim3(LM_THREADS), 0, s, bigram, ins, del, split, splits, run_costs,
                       piece_costs, first_run, n_of, slot, n_words, dec, chars, src, parts, static_cast<int32_t *>(margins), read_margin, cut_margin, read, alt, cut_alt,
                       edge_min, marginals);
}

} // namespace str_er
