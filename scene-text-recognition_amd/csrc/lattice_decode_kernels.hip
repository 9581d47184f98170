// lattice_decode_kernels.hip -- the joint decode of a word over its piece lattice and the bigram table on the device (gfx950):
// k_lattice_decode finds the cheapest path through the lattice of all pieces of all runs of every word together with the cheapest
// character string along it, with the optional DEL and INS moves, and backtracks both.  Integers only and no atomics: the output is the
// same bytes every time.  The rules are stated for the host in lattice_decode_rules.h; the contract is at str_er_lattice_decode in
// str_er.h.
//
// Built on k_word_decode (word_decode_device.h holds what the two share): a word per wave, LD_WORDS words per workgroup, the table
// staged once per workgroup in LDS with rows of 68 bytes, state a of V in lane a for a < 64, the states 64 and 65 in a second register
// of the lanes 0 and 1, the turned-round column for the target 64 and for the end of the word, values that travel with their state as
// keys (value << 7 | state: a value is below 2^21 -- at most 32 nodes of at most 5 * 255 each on top of INF = 2^20 -- so a key is below
// 2^28), one workgroup barrier and wave-level sync after it.
//
// The loop runs over the nodes 1 .. N of the word.  The min-plus product P_n[b] = min_a (V_n[a] + B[a][b]) depends on the source node
// alone, so it is made once, when node n is final, and kept for the up to three later nodes of the same run: no edge crosses a run
// boundary, so a ring of four (p0 .. p3, the local nodes 0 .. 3 of the current run; named registers, selected by compile-time indices
// in the unrolled loop over i) is enough, and a word costs N products like k_word_decode on N rows.  A target node then takes per edge
// the row byte, the penalty and two strict comparisons in the order the tie rule names -- i ascending, SUB before DEL -- while the
// smallest a comes with the product's key.  A back pointer carries i beside k_word_decode's 16 bits: 32-bit entries in LDS for 32
// nodes.  The backtrack runs on lane 0: it counts the parts from the end, and the sources and parts are turned to word order when they
// are written, once n_parts is known.  The parts go to the word's slot (the atoms of the words before it), which the host compacts.
//
// LDS per workgroup: 4488 (table) + 2 * 1088 (V and U keys) + 33792 (back pointers) + 512 (strings) + 128 (records) + 1664 (the nodes'
// runs and the parts) = 42760 bytes.
#include <hip/hip_runtime.h>

#include "lattice_decode_kernels.h"
#include "word_decode_device.h"

namespace str_er {

namespace {

constexpr int      LD_THREADS = 64 * LD_WORDS, LD_MAX_NODES = 32;
// a back pointer: k_word_decode's bits 0 .. 15 (the SUB predecessor, DEL, INS, the U-level state an inserted character follows) and in
// the bits 16, 17 the local node i the SUB or DEL move came from
constexpr int      LD_I_SHIFT = 16;

__device__ __forceinline__ int ld_wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the piece (i, j) of a run of A atoms in the order by (i, j) without (0, A); -1: the run itself
__device__ __forceinline__ int ld_piece_index(int A, int i, int j)
{
    if (i == 0) return j == A ? -1 : j - 1;
    return (A - 1) + (i - 1) * A - (i - 1) * i / 2 + (j - i - 1);
}

__device__ __forceinline__ int ld_atoms(const str_er_run_split *splits, int r) { return min(max(splits[r].n_cuts, 0), 3) + 1; }

// one edge into the node under construction: from the local node I with the product keys p (targets 0 .. 63, a lane each) and q (target
// 64), and the values v_lo / v_hi of V there; SUB first, then DEL, both strict
template <int I>
__device__ __forceinline__ void ld_edge(int lane, uint32_t p, uint32_t q, uint32_t v_lo, uint32_t v_hi, uint32_t cb, uint32_t c64, uint32_t s, uint32_t del,
                                        uint32_t &u_lo, uint32_t &u_hi, uint32_t &e_lo, uint32_t &e_hi)
{
    constexpr uint32_t at = (uint32_t)I << LD_I_SHIFT;
    const uint32_t s_lo = (p >> 7) + cb + s, s_hi = (q >> 7) + c64 + s;
    if (s_lo < u_lo) { u_lo = s_lo; e_lo = (p & 127u) | at; }
    if (lane == 0 && s_hi < u_hi) { u_hi = s_hi; e_hi = (q & 127u) | at; }
    if (del > 0) {
        if (v_lo + del + s < u_lo) { u_lo = v_lo + del + s; e_lo = WD_DEL | at; }
        if (v_hi + del + s < u_hi) { u_hi = v_hi + del + s; e_hi = WD_DEL | at; }
    }
}

__global__ void __launch_bounds__(LD_THREADS) k_lattice_decode(const uint8_t *__restrict__ bigram, int ins, int del, int split,
                                                               const str_er_run_split *__restrict__ splits, const uint8_t *__restrict__ run_costs,
                                                               const uint8_t *__restrict__ piece_costs, const int32_t *__restrict__ first_run,
                                                               const int32_t *__restrict__ n_of, const int32_t *__restrict__ slot, int n_words,
                                                               int32_t *__restrict__ dec, uint8_t *__restrict__ chars, uint8_t *__restrict__ src,
                                                               int32_t *__restrict__ parts)
{
    __shared__ __attribute__((aligned(16))) uint8_t  Bs[WD_STATES * WD_ROW];
    __shared__ __attribute__((aligned(16))) uint32_t vk[LD_WORDS][WD_ROW], uk[LD_WORDS][WD_ROW];
    __shared__ uint32_t bp[LD_WORDS][LD_MAX_NODES][WD_STATES];
    __shared__ uint8_t  out_c[LD_WORDS][64], out_s[LD_WORDS][64];
    __shared__ int32_t  rec[LD_WORDS][8];
    __shared__ int32_t  node_run[LD_WORDS][LD_MAX_NODES], part_run[LD_WORDS][LD_MAX_NODES], part_piece[LD_WORDS][LD_MAX_NODES];
    __shared__ uint8_t  node_ja[LD_WORDS][LD_MAX_NODES];          // the node's local index j | its run's atoms << 4
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t = tid; t < WD_STATES * WD_ROW; t += LD_THREADS) {
        const int a = t / WD_ROW, b = t - a * WD_ROW;
        Bs[t] = b < WD_STATES ? bigram[a * WD_STATES + b] : (uint8_t)0;
    }
    __syncthreads();          // (the only barrier of the workgroup: from here on a wave is on its own)
    const int w = (int)blockIdx.x * LD_WORDS + wave;
    if (w >= n_words) return;
    const int      first = __builtin_amdgcn_readfirstlane(first_run[w]), m = max(0, __builtin_amdgcn_readfirstlane(n_of[w]));
    const size_t   base = (size_t)__builtin_amdgcn_readfirstlane(slot[w]);
    uint32_t      *vkw = vk[wave], *ukw = uk[wave];
    const uint8_t *bcol = Bs + lane;
    int            prev = WD_E, N = 0;
    int32_t        rc = 0;
    for (int t = 0; t < m; t += 64) N += ld_wave_sum(t + lane < m ? ld_atoms(splits, first + t + lane) : 0);
    N = __builtin_amdgcn_readfirstlane(N);
    if (N > LD_MAX_NODES) {          // not decoded: the plain reading's cost alone
        for (int i = 0; i < m; ++i) {
            const uint8_t *row = run_costs + (size_t)(first + i) * WD_ALPHABET;
            wd_read_step(Bs, lane, row[lane], row[64], prev, rc);
        }
        if (lane == 0) {
            rec[wave][0] = -1; rec[wave][1] = rc + (int32_t)Bs[prev * WD_ROW + WD_E];
            rec[wave][2] = rec[wave][3] = rec[wave][4] = rec[wave][5] = rec[wave][6] = rec[wave][7] = 0;
        }
    } else {
        // V_0: the boundary at 0, every character at INF
        uint32_t key_lo = WD_INF << 7 | (uint32_t)lane;
        uint32_t key_hi = lane == 1 ? (uint32_t)WD_E : WD_INF << 7 | (uint32_t)(64 + (lane & 1));
        vkw[lane] = key_lo;
        if (lane < 2) vkw[64 + lane] = key_hi;
        // the ring: the products and the values of the local nodes 0 .. 3 of the current run
        uint32_t p0 = 0, p1 = 0, p2 = 0, p3 = 0, q0 = 0, q1 = 0, q2 = 0, q3 = 0;
        uint32_t vl0 = 0, vl1 = 0, vl2 = 0, vl3 = 0, vh0 = 0, vh1 = 0, vh2 = 0, vh3 = 0;
        int            r = first - 1, A = 0, j = 0, fp = 0;
        const uint8_t *rrow = run_costs;
        const uint32_t sp = (uint32_t)split, dl = (uint32_t)max(del, 0);
        for (int n = 1; n <= N; ++n) {
            wd_wave_sync();
            {          // the product of the node n - 1, final by now: local node 0 of a new run, or the local node j of the current one
                const uint32_t p = wd_product<WD_STATES>(vkw, key_lo, key_hi, bcol), q = wd_column(Bs, lane, 64, key_lo, key_hi, 2);
                const uint32_t v_lo = key_lo >> 7, v_hi = key_hi >> 7;
                if (j == A) {
                    ++r;
                    A = __builtin_amdgcn_readfirstlane(ld_atoms(splits, r)); fp = __builtin_amdgcn_readfirstlane(splits[r].first_piece);
                    rrow = run_costs + (size_t)r * WD_ALPHABET;
                    j = 0;
                    p0 = p; q0 = q; vl0 = v_lo; vh0 = v_hi;
                } else if (j == 1) { p1 = p; q1 = q; vl1 = v_lo; vh1 = v_hi; }
                else if (j == 2) { p2 = p; q2 = q; vl2 = v_lo; vh2 = v_hi; }
                else { p3 = p; q3 = q; vl3 = v_lo; vh3 = v_hi; }
            }
            ++j;
            uint32_t u_lo = WD_INF, u_hi = WD_INF, e_lo = 0, e_hi = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < j) {
                    const int      k = ld_piece_index(A, i, j);
                    const uint8_t *row = k < 0 ? rrow : piece_costs + ((size_t)fp + (size_t)k) * WD_ALPHABET;
                    const uint32_t cb = row[lane], c64 = row[64], s = i > 0 ? sp : 0u;
                    if (k < 0) wd_read_step(Bs, lane, cb, c64, prev, rc);          // (the run's own row: a step of the plain reading)
                    if (i == 0) ld_edge<0>(lane, p0, q0, vl0, vh0, cb, c64, s, dl, u_lo, u_hi, e_lo, e_hi);
                    else if (i == 1) ld_edge<1>(lane, p1, q1, vl1, vh1, cb, c64, s, dl, u_lo, u_hi, e_lo, e_hi);
                    else if (i == 2) ld_edge<2>(lane, p2, q2, vl2, vh2, cb, c64, s, dl, u_lo, u_hi, e_lo, e_hi);
                    else ld_edge<3>(lane, p3, q3, vl3, vh3, cb, c64, s, dl, u_lo, u_hi, e_lo, e_hi);
                }
            uint32_t w_lo = u_lo, w_hi = u_hi;
            if (ins > 0) {
                const uint32_t uk_lo = u_lo << 7 | (uint32_t)lane, uk_hi = u_hi << 7 | 64u;          // (uk_hi counts in lane 0 alone)
                ukw[lane] = uk_lo;
                if (lane == 0) ukw[64] = uk_hi;
                wd_wave_sync();
                const uint32_t i_lo = wd_product<WD_ALPHABET>(ukw, uk_lo, uk_hi, bcol);
                const uint32_t i_64 = wd_column(Bs, lane, 64, uk_lo, uk_hi, 1);
                if ((i_lo >> 7) + (uint32_t)ins < u_lo) { w_lo = (i_lo >> 7) + (uint32_t)ins; e_lo |= WD_INS | (i_lo & 127u) << 9; }
                if (lane == 0 && (i_64 >> 7) + (uint32_t)ins < u_hi) { w_hi = (i_64 >> 7) + (uint32_t)ins; e_hi |= WD_INS | (i_64 & 127u) << 9; }
            }
            key_lo = w_lo << 7 | (uint32_t)lane;
            key_hi = w_hi << 7 | (uint32_t)(64 + (lane & 1));
            vkw[lane] = key_lo;
            bp[wave][n - 1][lane] = e_lo;
            if (lane < 2) { vkw[64 + lane] = key_hi; bp[wave][n - 1][64 + lane] = e_hi; }
            if (lane == 0) { node_run[wave][n - 1] = r; node_ja[wave][n - 1] = (uint8_t)(j | A << 4); }
        }
        const uint32_t end = wd_column(Bs, lane, WD_E, key_lo, key_hi, 2);
        wd_wave_sync();
        if (lane == 0) {          // the backtrack: the string and the parts from their ends, a source counts the parts from the end
            int state = (int)(end & 127u), at = 64, n_sub = 0, n_del = 0, n_ins = 0, np = 0;
            for (int n = N; n >= 1;) {
                const uint32_t *st = bp[wave][n - 1];
                uint32_t        e = st[state];
                if (e & WD_INS) {
                    out_c[wave][--at] = (uint8_t)state; out_s[wave][at] = (uint8_t)(np | 0x80);
                    ++n_ins;
                    state = (int)(e >> 9 & 127u);
                    e = st[state];
                }
                const int run = node_run[wave][n - 1], nj = node_ja[wave][n - 1] & 15, nA = node_ja[wave][n - 1] >> 4, i = (int)(e >> LD_I_SHIFT & 3u);
                const int k = ld_piece_index(nA, i, nj);
                part_run[wave][np] = run; part_piece[wave][np] = k < 0 ? -1 : splits[run].first_piece + k;
                if (e & WD_DEL) ++n_del;
                else {
                    out_c[wave][--at] = (uint8_t)state; out_s[wave][at] = (uint8_t)np;
                    ++n_sub;
                    state = (int)(e & 127u);
                }
                ++np;
                n -= max(nj - i, 1);
            }
            rec[wave][0] = (int32_t)(end >> 7); rec[wave][1] = rc + (int32_t)Bs[prev * WD_ROW + WD_E];
            rec[wave][2] = 64 - at; rec[wave][3] = n_sub; rec[wave][4] = n_del; rec[wave][5] = n_ins; rec[wave][6] = 0; rec[wave][7] = np;
        }
    }
    wd_wave_sync();
    const int n_chars = rec[wave][2], n_parts = rec[wave][7];
    const int from = 64 - n_chars + lane;          // (n_chars <= 64: the string sits at the end of out_c)
    const uint32_t sb = lane < n_chars ? out_s[wave][from] : 0u;
    chars[(size_t)w * 64 + lane] = lane < n_chars ? out_c[wave][from] : (uint8_t)0xFF;
    src[(size_t)w * 64 + lane] = lane < n_chars ? (uint8_t)(((uint32_t)(n_parts - 1) - (sb & 127u)) | (sb & 128u)) : (uint8_t)0xFF;
    if (lane < n_parts) {          // (n_parts <= N <= 32, the slots of the word)
        parts[2 * (base + (size_t)lane)] = part_run[wave][n_parts - 1 - lane];
        parts[2 * (base + (size_t)lane) + 1] = part_piece[wave][n_parts - 1 - lane];
    }
    if (lane < 8) dec[(size_t)w * 8 + lane] = rec[wave][lane];
}

} // namespace

void launch_lattice_decode(hipStream_t s, const uint8_t *bigram, int ins, int del, int split, const str_er_run_split *splits, const uint8_t *run_costs,
                           const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of, const int32_t *slot, int n_words, int32_t *dec, uint8_t *chars,
                           uint8_t *src, int32_t *parts)
{
    if (n_words <= 0) return;
    hipLaunchKernelGGL(k_lattice_decode, dim3((unsigned)((n_words + LD_WORDS - 1) / LD_WORDS)), dim3(LD_THREADS), 0, s, bigram, ins, del, split, splits, run_costs,
                       piece_costs, first_run, n_of, slot, n_words, dec, chars, src, parts);
}

} // namespace str_er
