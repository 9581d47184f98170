// lattice_match_kernels.hip -- the lexicon match of a word over its piece lattice on the device (gfx950): k_lattice_match runs the
// weighted edit distance of every lexicon entry in the word's band of lengths over the lattice of all pieces of all runs of the word
// and keeps the two smallest (cost, index) keys per (word, chunk); k_lattice_match_final merges a word's chunks, makes free_cost and
// n_tried, and runs the whole table of the winning entry once to backtrack its parts and sources.  Integers only and no atomics: the
// output is the same bytes every time.  The rules are stated for the host in lattice_match_rules.h; the contract is at
// str_er_lattice_match in str_er.h.
//
// k_lattice_match is k_word_match (word_match_kernels.hip) with up to four predecessors a node: grid (chunks, words) on the matcher's
// lexicon, a wave 64 entries of one length, a lane an entry, the column D[0 .. MC][j] over the nodes in registers with every index a
// compile-time constant (node buckets of 8 / 16 / 32).  The workgroup stages the rows of the word's edges in LDS (at most 80 rows of 65
// bytes: 8 runs of 4 atoms), folded where the lexicon folds, each at the slot of the node it ends at and of its span d = 1 .. 4 (slot
// 4 (n - 1) + d - 1), so that the address of a row byte is the character plus a compile-time offset as in the matcher.  What is left of
// the word's structure is the local index jl of every node, two bits each: two scalar registers for 32 nodes.  It is the same for every
// lane, so every branch on it is uniform: a node with jl = 1 takes the matcher's cell after one branch, and a word without any cut runs
// the matcher's own loop (wm_entry_cost) on rows staged back to back.  A node step reads one byte per edge; the old values of the four
// nodes before it travel in four registers (renamed by the unrolled loop, not moved).  The minimum needs no order: the order of the
// candidates matters to the backtrack alone, which k_lattice_match_final does.
//
// k_lattice_match_final takes a wave per word: lane j holds the column j of the table, a node's INS chain is a prefix minimum over the
// lanes (D[n][j] = j INS + min over k <= j of (X[k] - k INS), X the best SUB / DEL candidate), the table and the byte every (node, edge,
// character) read cost are kept in LDS, and lane 0 walks back through them.
#include <hip/hip_runtime.h>

#include "lattice_match_kernels.h"
#include "lattice_match_device.h"

namespace str_er {

namespace {

constexpr int LM_THREADS = 256, LM_WAVES = LM_THREADS / 64;

// The groups [g0, g1) of one chunk against the word staged in ct / node_s / d0: a wave takes every LM_WAVES-th group, a lane one entry.
// A word without a cut is a sequence of rows: its rows are staged back to back and the matcher's own cell loop runs on them.
template <int MC>
__device__ __forceinline__ void lm_chunk(const WmLexDev &lex, const uint8_t *ct, const uint32_t *node_s, const int *d0, int g0, int g1, int len_lo, int N, int ins, int del,
                                         int split, uint64_t &k1, uint64_t &k2)
{
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const uint32_t S0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)node_s[0]), S1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)node_s[1]);
    const bool     cut = (S0 | S1) != 0;
    for (int g = g0 + wave; g < g1; g += LM_WAVES) {
        const int gu = __builtin_amdgcn_readfirstlane(g);
        int       len = len_lo;
        while (gu >= lex.len_first[len + 1]) ++len;          // (gu < g1 <= len_first[len_hi + 1]: it ends inside the table)
        const int32_t   idx = lex.index[(size_t)gu * WM_GROUP + lane];
        const uint32_t *words = lex.chars + lex.goff[gu] + lane;
        const int       c = cut ? lm_entry_cost<MC>(ct, S0, S1, d0, words, len, N, ins, del, split) : wm_entry_cost<MC>(ct, words, len, N, ins, del);
        if (idx >= 0) wm_add(k1, k2, (uint64_t)(uint32_t)c << 32 | (uint32_t)idx);
    }
}

// grid (chunks, words).  The word's structure is uniform per workgroup and the length per wave.
__global__ void __launch_bounds__(LM_THREADS) k_lattice_match(WmLexDev lex, WmParams prm, int split, const str_er_run_split *__restrict__ splits,
                                                              const uint8_t *__restrict__ run_costs, const uint8_t *__restrict__ piece_costs,
                                                              const int32_t *__restrict__ first_run, const int32_t *__restrict__ n_of, uint64_t *__restrict__ partial)
{
    __shared__ uint8_t  ct[LM_SLOTS * WM_ALPHABET];
    __shared__ uint32_t node_s[2];
    __shared__ int      d0[LM_MAX_NODES + 1];
    __shared__ int32_t  erow[LM_SLOTS];
    __shared__ int32_t  r_atoms[LM_MAX_RUNS], r_fp[LM_MAX_RUNS];
    __shared__ int32_t  hdr[1];
    __shared__ uint64_t wk[LM_WAVES][2];
    const int w = (int)blockIdx.y, chunk = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int m = max(n_of[w], 0), first = first_run[w], mr = min(m, LM_MAX_RUNS);
    uint64_t *out = partial + ((size_t)w * gridDim.x + chunk) * 2;
    if (tid < mr) { r_atoms[tid] = lm_atoms(splits, first + tid); r_fp[tid] = splits[first + tid].first_piece; }
    __syncthreads();
    if (tid < LM_SLOTS) erow[tid] = -1;
    __syncthreads();
    if (tid == 0) {          // the structure: the nodes' local indices, the rows of the slots and the column D[n][0]
        int      N = 0;
        uint32_t sw[2] = {0, 0};
        d0[0] = 0;
        for (int t = 0; t < mr; ++t) {
            const int A = r_atoms[t], fp = r_fp[t];
            if (N + A > LM_MAX_NODES) { N = LM_MAX_NODES + 1; break; }
            for (int jl = 1; jl <= A; ++jl) {
                const int n = N + jl;
                int       dn = 0x7FFFFFFF;
                sw[(n - 1) >> 4] |= (uint32_t)(jl - 1) << (2 * ((n - 1) & 15));
                for (int d = 1; d <= jl; ++d) {
                    const int i = jl - d, k = lm_piece_index(A, i, jl);
                    erow[(n - 1) * 4 + d - 1] = k < 0 ? first + t : (fp + k) | LM_PIECE;
                    dn = min(dn, d0[n - d] + prm.del + (i > 0 ? split : 0));
                }
                d0[n] = dn;
            }
            N += A;
        }
        if (m > mr) N = LM_MAX_NODES + 1;
        for (int n = N + 1; n <= LM_MAX_NODES; ++n) d0[n] = 0;      // (past N: jl = 1, computed and not used)
        node_s[0] = sw[0]; node_s[1] = sw[1];
        hdr[0] = N;
    }
    __syncthreads();
    const int N = hdr[0];
    const int len_lo = max(1, m - prm.band), len_hi = min(32, N + prm.band);
    int       g0 = 0, g1 = 0;
    if (N <= LM_MAX_NODES && len_lo <= len_hi) {
        g0 = lex.len_first[len_lo] + chunk * WM_CHUNK_GROUPS;
        g1 = min(lex.len_first[len_hi + 1], g0 + WM_CHUNK_GROUPS);
    }
    if (g0 >= g1) {          // (uniform: nothing of this word in this chunk)
        if (tid == 0) { out[0] = WM_NO_KEY; out[1] = WM_NO_KEY; }
        return;
    }
    // the rows of the word's edges into their slots in LDS, folded where the lexicon folds case; a slot without an edge costs 255 (only
    // the nodes past N read one, and they are not used).  A word without a cut has one edge a node: its rows lie back to back, as the
    // matcher lays them out
    const int  MC = N <= 8 ? 8 : N <= 16 ? 16 : 32;
    const bool cut = (node_s[0] | node_s[1]) != 0;
    for (int t = tid; t < (cut ? MC * 4 : MC) * WM_ALPHABET; t += LM_THREADS) {
        const int     k = t / WM_ALPHABET, a = t - k * WM_ALPHABET;
        const int32_t at = erow[cut ? k : 4 * k];
        int           v = 255;
        if (at >= 0) {
            const uint8_t *C = at & LM_PIECE ? piece_costs + (size_t)(at & (LM_PIECE - 1)) * WM_ALPHABET : run_costs + (size_t)at * WM_ALPHABET;
            v = C[a];
            if (lex.fold) v = min(v, (int)C[wm_partner(a)]);
        }
        ct[t] = (uint8_t)v;
    }
    __syncthreads();
    uint64_t k1 = WM_NO_KEY, k2 = WM_NO_KEY;
    if (MC == 8) lm_chunk<8>(lex, ct, node_s, d0, g0, g1, len_lo, N, prm.ins, prm.del, split, k1, k2);
    else if (MC == 16) lm_chunk<16>(lex, ct, node_s, d0, g0, g1, len_lo, N, prm.ins, prm.del, split, k1, k2);
    else lm_chunk<32>(lex, ct, node_s, d0, g0, g1, len_lo, N, prm.ins, prm.del, split, k1, k2);
    // the wave's two smallest by a butterfly (every lane ends with them), the workgroup's through LDS
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t o1 = wm_shfl_xor(k1, off), o2 = wm_shfl_xor(k2, off);
        const uint64_t lo = min(k1, o1), hi = max(k1, o1);
        k2 = min(hi, min(k2, o2));
        k1 = lo;
    }
    if ((tid & 63) == 0) { wk[tid >> 6][0] = k1; wk[tid >> 6][1] = k2; }
    __syncthreads();
    if (tid == 0) {
        uint64_t b1 = WM_NO_KEY, b2 = WM_NO_KEY;
        for (int v = 0; v < LM_WAVES; ++v) { wm_add(b1, b2, wk[v][0]); wm_add(b1, b2, wk[v][1]); }
        out[0] = b1; out[1] = b2;
    }
}

// ---- k_lattice_match_final --------------------------------------------------------------------------------------------------------
// a wave per word
__global__ void __launch_bounds__(64 * LM_FINAL_WORDS) k_lattice_match_final(WmLexDev lex, WmParams prm, int split, const str_er_run_split *__restrict__ splits,
                                                                             const uint8_t *__restrict__ run_costs, const uint8_t *__restrict__ piece_costs,
                                                                             const int32_t *__restrict__ first_run, const int32_t *__restrict__ n_of,
                                                                             const int32_t *__restrict__ slot, int n_words, int n_chunks,
                                                                             const uint64_t *__restrict__ partial, int32_t *__restrict__ matches,
                                                                             uint8_t *__restrict__ src, int32_t *__restrict__ parts)
{
    __shared__ LmWaveLds lds[LM_FINAL_WORDS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = (int)blockIdx.x * LM_FINAL_WORDS + wave;
    if (w >= n_words) return;          // (no workgroup barrier below: a wave is on its own)
    const int    first = __builtin_amdgcn_readfirstlane(first_run[w]), m = max(0, __builtin_amdgcn_readfirstlane(n_of[w]));
    const size_t base = (size_t)__builtin_amdgcn_readfirstlane(slot[w]);
    // the chunks' pairs merged (NO_KEY never displaces a key)
    uint64_t b1 = WM_NO_KEY, b2 = WM_NO_KEY;
    for (int ch = lane; ch < n_chunks; ch += 64) {
        const uint64_t *p = partial + ((size_t)w * n_chunks + ch) * 2;
        wm_add(b1, b2, p[0]);
        wm_add(b1, b2, p[1]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t o1 = wm_shfl_xor(b1, off), o2 = wm_shfl_xor(b2, off);
        const uint64_t lo = min(b1, o1), hi = max(b1, o1);
        b2 = min(hi, min(b2, o2));
        b1 = lo;
    }
    // the runs one after the other: the free segmentation of each on the minima of its rows, and the nodes while they are at most 32
    LmWaveLds    &L = lds[wave];
    int           N = 0;
    const int32_t fc = lm_wave_nodes(L, splits, run_costs, piece_costs, first, m, split, lane, N);
    const int  len_lo = max(1, m - prm.band), len_hi = min(32, N + prm.band);
    const bool tried = N <= LM_MAX_NODES && len_lo <= len_hi;
    const int  entry = b1 == WM_NO_KEY ? -1 : (int)(uint32_t)b1;
    const int  len = lm_wave_winner(L, lex, prm, split, run_costs, piece_costs, entry, N, entry >= 0 && tried, lane);
    lm_wave_sync();
    lm_wave_store(L, len, lane, src + (size_t)w * 32, parts + 2 * base);
    if (lane == 0) {
        int32_t *o = matches + (size_t)w * 10;
        o[0] = entry;
        o[1] = b1 == WM_NO_KEY ? -1 : (int32_t)(b1 >> 32);
        o[2] = b2 == WM_NO_KEY ? -1 : (int32_t)(uint32_t)b2;
        o[3] = b2 == WM_NO_KEY ? -1 : (int32_t)(b2 >> 32);
        o[4] = fc;
        o[5] = tried ? lex.len_count[len_hi + 1] - lex.len_count[len_lo] : 0;
        o[6] = 0; o[7] = L.rec[0]; o[8] = L.rec[1]; o[9] = L.rec[2];
    }
}

} // namespace

void launch_lattice_match(hipStream_t s, const WmLexDev &lex, const WmParams &p, int split, const str_er_run_split *splits, const uint8_t *run_costs,
                          const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of, const int32_t *slot, int n_words, uint64_t *partial,
                          int32_t *matches, uint8_t *src, int32_t *parts)
{
    if (n_words <= 0) return;
    const int n_chunks = wm_chunks(lex);
    // (the words are the grid's y: at most 65535 a launch)
    for (int w0 = 0; w0 < n_words; w0 += 65535) {
        const int nw = std::min(65535, n_words - w0);
        hipLaunchKernelGGL(k_lattice_match, dim3((unsigned)n_chunks, (unsigned)nw), dim3(LM_THREADS), 0, s, lex, p, split, splits, run_costs, piece_costs, first_run + w0,
                           n_of + w0, partial + (size_t)w0 * n_chunks * 2);
    }
    hipLaunchKernelGGL(k_lattice_match_final, dim3((unsigned)((n_words + LM_FINAL_WORDS - 1) / LM_FINAL_WORDS)), dim3(64 * LM_FINAL_WORDS), 0, s, lex, p, split, splits,
                       run_costs, piece_costs, first_run, n_of, slot, n_words, n_chunks, partial, matches, src, parts);
}

} // namespace str_er
