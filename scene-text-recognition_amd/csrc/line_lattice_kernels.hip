// line_lattice_kernels.hip -- the joint decode of a text line over the piece lattices of its runs on the device (gfx950):
// k_line_lattice_decode finds the cheapest path through the atoms' ends of all runs of every line -- the cuts of touching glyphs, the
// word breaks and the string together -- and backtracks it.  Integers only and no atomics: the output is the same bytes every time.
// The rules are stated for the host in line_lattice_rules.h; the contract is at str_er_line_lattice_decode in str_er.h.
//
// Built from its two parents (word_decode_device.h holds what they share).  A line per wave, LL_LINES lines per workgroup, the table
// staged once per workgroup in LDS with rows of 68 bytes, state a of V in lane a for a < 64, the states 64 and 65 in a second register
// of the lanes 0 and 1, a value with its state as a key (value << 7 | state: a value is below 2^25, line_lattice_rules.h), one
// workgroup barrier and wave-level sync after it.  The loop runs over the nodes 1 .. N of the line as k_lattice_decode's does over a
// word's: the min-plus product of a node is made once, when the node is final, and kept in a ring of four named registers (the local
// nodes 0 .. 3 of the current run, selected by compile-time indices in the unrolled loop over i).  Where a new run begins that is not
// the line's first, the gap step of k_line_decode comes before the product of its local node 0: one more turned-round column, the one
// of the end of a word, the join added to both key registers, and lane 1 alone -- E lives there -- compares break and join.  A line
// has up to 4096 nodes, so nothing per node fits LDS: the back pointers go to a scratch table in device memory, 68 uint32 a node (the
// node step's word of the states 0 .. 65 in k_lattice_decode's encoding, the gap's break | predecessor at the run's first node, the
// node's (j, A, run)), which only this wave reads again.  Lane 0 backtracks into the tails of the line's slices, counting the parts
// from the end; then the wave moves labels, sources, parts and the parts' words to the front of the slices in chunks of 64 entries,
// ascending -- the destination lies below the source -- and turns the part indices and the words round.  The chain over the nodes is
// serial per line: the kernel's time is the longest line's (profiles/line_lattice_decode.md).
//
// LDS per workgroup: 4488 (table) + 2 * 1088 (V and U keys) + 128 (records) = 6792 bytes, 6800 as the compiler lays them out (the key
// vectors are aligned to 16 bytes behind the table).
#include <hip/hip_runtime.h>

#include "line_lattice_kernels.h"
#include "word_decode_device.h"

namespace str_er {

namespace {

constexpr int      LL_THREADS = 64 * LL_LINES, LL_MAX_RUNS = 1024, LL_GAP = 66, LL_NODE = 67;
constexpr uint32_t LL_OFF = 255, LL_BREAK = 1u << 7;
// a back pointer: k_word_decode's bits 0 .. 15 (the SUB predecessor, DEL, INS, the U-level state an inserted character follows) and in
// the bits 16, 17 the local node i the SUB or DEL move came from
constexpr int      LL_I_SHIFT = 16;

__device__ __forceinline__ int ll_wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the piece (i, j) of a run of A atoms in the order by (i, j) without (0, A); -1: the run itself
__device__ __forceinline__ int ll_piece_index(int A, int i, int j)
{
    if (i == 0) return j == A ? -1 : j - 1;
    return (A - 1) + (i - 1) * A - (i - 1) * i / 2 + (j - i - 1);
}

__device__ __forceinline__ int ll_atoms(const str_er_run_split *splits, int r) { return min(max(splits[r].n_cuts, 0), 3) + 1; }

// one edge into the node under construction: from the local node I with the product keys p (targets 0 .. 63, a lane each) and q (target
// 64), and the values v_lo / v_hi of V there; SUB first, then DEL, both strict
template <int I>
__device__ __forceinline__ void ll_edge(int lane, uint32_t p, uint32_t q, uint32_t v_lo, uint32_t v_hi, uint32_t cb, uint32_t c64, uint32_t s, uint32_t del,
                                        uint32_t &u_lo, uint32_t &u_hi, uint32_t &e_lo, uint32_t &e_hi)
{
    constexpr uint32_t at = (uint32_t)I << LL_I_SHIFT;
    const uint32_t s_lo = (p >> 7) + cb + s, s_hi = (q >> 7) + c64 + s;
    if (s_lo < u_lo) { u_lo = s_lo; e_lo = (p & 127u) | at; }
    if (lane == 0 && s_hi < u_hi) { u_hi = s_hi; e_hi = (q & 127u) | at; }
    if (del > 0) {
        if (v_lo + del + s < u_lo) { u_lo = v_lo + del + s; e_lo = WD_DEL | at; }
        if (v_hi + del + s < u_hi) { u_hi = v_hi + del + s; e_hi = WD_DEL | at; }
    }
}

__global__ void __launch_bounds__(LL_THREADS) k_line_lattice_decode(const uint8_t *__restrict__ bigram, int ins, int del, int split,
                                                                    const str_er_run_split *__restrict__ splits, const uint8_t *__restrict__ run_costs,
                                                                    const uint8_t *__restrict__ piece_costs, const uint8_t *__restrict__ gaps,
                                                                    const int32_t *__restrict__ first_run, const int32_t *__restrict__ n_of,
                                                                    const int32_t *__restrict__ slot, int n_lines, uint32_t *bp, int32_t *__restrict__ dec,
                                                                    uint8_t *chars, uint16_t *src, int32_t *parts, int32_t *word_of_part)
{
    __shared__ __attribute__((aligned(16))) uint8_t  Bs[WD_STATES * WD_ROW];
    __shared__ __attribute__((aligned(16))) uint32_t vk[LL_LINES][WD_ROW], uk[LL_LINES][WD_ROW];
    __shared__ int32_t  rec[LL_LINES][8];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t = tid; t < WD_STATES * WD_ROW; t += LL_THREADS) {
        const int a = t / WD_ROW, b = t - a * WD_ROW;
        Bs[t] = b < WD_STATES ? bigram[a * WD_STATES + b] : (uint8_t)0;
    }
    __syncthreads();          // (the only barrier of the workgroup: from here on a wave is on its own)
    const int line = (int)blockIdx.x * LL_LINES + wave;
    if (line >= n_lines) return;
    const int    first = __builtin_amdgcn_readfirstlane(first_run[line]), m = max(0, __builtin_amdgcn_readfirstlane(n_of[line]));
    const size_t base = (size_t)__builtin_amdgcn_readfirstlane(slot[line]);
    int          N = 0;
    for (int t = 0; t < m; t += 64) N += ll_wave_sum(t + lane < m ? ll_atoms(splits, first + t + lane) : 0);
    N = __builtin_amdgcn_readfirstlane(N);
    uint8_t  *oc = chars + 3 * base;
    uint16_t *os = src + 3 * base;
    int32_t  *pt = parts + 2 * base, *wp = word_of_part + base;
    if (m > LL_MAX_RUNS) {          // not decoded
        for (int k = lane; k < 3 * N; k += 64) { oc[k] = (uint8_t)0xFF; os[k] = (uint16_t)0xFFFF; }
        for (int k = lane; k < N; k += 64) { pt[2 * k] = -1; pt[2 * k + 1] = -1; wp[k] = -1; }
        if (lane < 8) dec[(size_t)line * 8 + lane] = lane == 0 ? -1 : 0;
        return;
    }
    uint32_t      *bpl = bp + base * LL_BP_ROW;
    uint32_t      *vkw = vk[wave], *ukw = uk[wave];
    const uint8_t *bcol = Bs + lane;
    // V_0: the boundary at 0, every character at INF
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
        const uint32_t sp = (uint32_t)split, dl = (uint32_t)max(del, 0);
        for (int n = 1; n <= N; ++n) {
            uint32_t  *st = bpl + (size_t)(n - 1) * LL_BP_ROW;
            const bool fresh = j == A;          // (the same in every lane: node n - 1 is local node 0 of a new run)
            if (fresh) {
                ++r;
                A = __builtin_amdgcn_readfirstlane(ll_atoms(splits, r)); fp = __builtin_amdgcn_readfirstlane(splits[r].first_piece);
                rrow = run_costs + (size_t)r * WD_ALPHABET;
                if (r > first) {          // the gap in front of the run: every state joins, the boundary may come from a break
                    const uint32_t J = (uint32_t)__builtin_amdgcn_readfirstlane((int)gaps[2 * (size_t)r]),
                                   K = (uint32_t)__builtin_amdgcn_readfirstlane((int)gaps[2 * (size_t)r + 1]);
                    const uint32_t x = wd_column(Bs, lane, WD_E, key_lo, key_hi, 2);
                    if (J == LL_OFF) {
                        key_lo = WD_INF << 7 | (uint32_t)lane;
                        key_hi = WD_INF << 7 | (uint32_t)(64 + (lane & 1));
                    } else {
                        key_lo += J << 7; key_hi += J << 7;
                    }
                    if (lane == 1) {
                        uint32_t g = 0;
                        if (K != LL_OFF && (x >> 7) + K < key_hi >> 7) { key_hi = ((x >> 7) + K) << 7 | (uint32_t)WD_E; g = LL_BREAK | (x & 127u); }
                        st[LL_GAP] = g;
                    }
                    vkw[lane] = key_lo;
                    if (lane < 2) vkw[64 + lane] = key_hi;
                }
            }
            wd_wave_sync();
            {          // the product of the node n - 1, final by now: local node 0 of a new run (behind its gap), or the local node j of the current one
                const uint32_t p = wd_product<WD_STATES>(vkw, key_lo, key_hi, bcol), q = wd_column(Bs, lane, 64, key_lo, key_hi, 2);
                const uint32_t v_lo = key_lo >> 7, v_hi = key_hi >> 7;
                if (fresh) { j = 0; p0 = p; q0 = q; vl0 = v_lo; vh0 = v_hi; }
                else if (j == 1) { p1 = p; q1 = q; vl1 = v_lo; vh1 = v_hi; }
                else if (j == 2) { p2 = p; q2 = q; vl2 = v_lo; vh2 = v_hi; }
                else { p3 = p; q3 = q; vl3 = v_lo; vh3 = v_hi; }
            }
            ++j;
            uint32_t u_lo = WD_INF, u_hi = WD_INF, e_lo = 0, e_hi = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < j) {
                    const int      k = ll_piece_index(A, i, j);
                    const uint8_t *row = k < 0 ? rrow : piece_costs + ((size_t)fp + (size_t)k) * WD_ALPHABET;
                    const uint32_t cb = row[lane], c64 = row[64], s = i > 0 ? sp : 0u;
                    if (i == 0) ll_edge<0>(lane, p0, q0, vl0, vh0, cb, c64, s, dl, u_lo, u_hi, e_lo, e_hi);
                    else if (i == 1) ll_edge<1>(lane, p1, q1, vl1, vh1, cb, c64, s, dl, u_lo, u_hi, e_lo, e_hi);
                    else if (i == 2) ll_edge<2>(lane, p2, q2, vl2, vh2, cb, c64, s, dl, u_lo, u_hi, e_lo, e_hi);
                    else ll_edge<3>(lane, p3, q3, vl3, vh3, cb, c64, s, dl, u_lo, u_hi, e_lo, e_hi);
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
            st[lane] = e_lo;
            if (lane < 2) { vkw[64 + lane] = key_hi; st[64 + lane] = e_hi; }
            if (lane == 0) st[LL_NODE] = (uint32_t)j | (uint32_t)A << 4 | (uint32_t)(r - first) << 8;
        }
    }
    const uint32_t end = wd_column(Bs, lane, WD_E, key_lo, key_hi, 2);
    wd_global_sync();
    if (lane == 0) {          // the backtrack: the string, the parts and their words from their ends, into the tails of the line's slices
        int state = (int)(end & 127u), at = 3 * N, np = 0, n_sub = 0, n_del = 0, n_ins = 0, n_brk = 0;
        for (int n = N; n >= 1;) {
            const uint32_t *st = bpl + (size_t)(n - 1) * LL_BP_ROW;
            uint32_t        e = st[state];
            if (e & WD_INS) {
                oc[--at] = (uint8_t)state; os[at] = (uint16_t)(np | 0x8000);
                ++n_ins;
                state = (int)(e >> 9 & 127u);
                e = st[state];
            }
            const uint32_t nd = st[LL_NODE];
            const int      nj = (int)(nd & 15u), nA = (int)(nd >> 4 & 15u), rr = (int)(nd >> 8), i = (int)(e >> LL_I_SHIFT & 3u);
            const int      k = ll_piece_index(nA, i, nj);
            pt[2 * (N - 1 - np)] = first + rr; pt[2 * (N - 1 - np) + 1] = k < 0 ? -1 : splits[first + rr].first_piece + k;
            if (e & WD_DEL) { ++n_del; wp[N - 1 - np] = -1; }
            else {
                oc[--at] = (uint8_t)state; os[at] = (uint16_t)np;
                wp[N - 1 - np] = n_brk;          // (the breaks behind it: turned round below)
                ++n_sub;
                state = (int)(e & 127u);
            }
            ++np;
            if (i == 0 && rr > 0 && state == WD_E) {          // local node 0 of a run at the boundary: the gap's word lies at the run's first node
                const uint32_t g = bpl[(size_t)(n - nj) * LL_BP_ROW + LL_GAP];
                if (g & LL_BREAK) {
                    oc[--at] = (uint8_t)WD_E; os[at] = (uint16_t)((np - 1) | 0x4000);
                    ++n_brk;
                    state = (int)(g & 127u);
                }
            }
            n -= max(nj - i, 1);
        }
        rec[wave][0] = (int32_t)(end >> 7); rec[wave][1] = 3 * N - at; rec[wave][2] = n_brk; rec[wave][3] = n_sub;
        rec[wave][4] = n_del; rec[wave][5] = n_ins; rec[wave][6] = 0; rec[wave][7] = np;
    }
    wd_global_sync();
    const int n_chars = rec[wave][1], n_brk = rec[wave][2], np = rec[wave][7], from = 3 * N - n_chars, pfrom = N - np;
    for (int c0 = 0; c0 < n_chars; c0 += 64) {          // ascending: chunk c is written below everything a later chunk reads
        const int k = c0 + lane;
        uint8_t   ch = 0;
        uint32_t  sv = 0;
        if (k < n_chars) { ch = oc[from + k]; sv = os[from + k]; }
        wd_global_sync();
        if (k < n_chars) { oc[k] = ch; os[k] = (uint16_t)(((uint32_t)(np - 1) - (sv & 0x3FFFu)) | (sv & 0xC000u)); }
    }
    for (int c0 = 0; c0 < np; c0 += 64) {          // the parts and their words lie in line order already: moved alike
        const int k = c0 + lane;
        int32_t   pr = 0, pp = 0, v = 0;
        if (k < np) { pr = pt[2 * (pfrom + k)]; pp = pt[2 * (pfrom + k) + 1]; v = wp[pfrom + k]; }
        wd_global_sync();
        if (k < np) { pt[2 * k] = pr; pt[2 * k + 1] = pp; wp[k] = v >= 0 ? n_brk - v : -1; }
    }
    wd_global_sync();
    for (int k = n_chars + lane; k < 3 * N; k += 64) { oc[k] = (uint8_t)0xFF; os[k] = (uint16_t)0xFFFF; }
    for (int k = np + lane; k < N; k += 64) { pt[2 * k] = -1; pt[2 * k + 1] = -1; wp[k] = -1; }
    if (lane < 8) dec[(size_t)line * 8 + lane] = rec[wave][lane];
}

} // namespace

void launch_line_lattice_decode(hipStream_t s, const uint8_t *bigram, int ins, int del, int split, const str_er_run_split *splits, const uint8_t *run_costs,
                                const uint8_t *piece_costs, const uint8_t *gaps, const int32_t *first_run, const int32_t *n_of, const int32_t *slot, int n_lines,
                                uint32_t *bp, int32_t *dec, uint8_t *chars, uint16_t *src, int32_t *parts, int32_t *word_of_part)
{
    if (n_lines <= 0) return;
    hipLaunchKernelGGL(k_line_lattice_decode, dim3((unsigned)((n_lines + LL_LINES - 1) / LL_LINES)), dim3(LL_THREADS), 0, s, bigram, ins, del, split, splits,
                       run_costs, piece_costs, gaps, first_run, n_of, slot, n_lines, bp, dec, chars, src, parts, word_of_part);
}

} // namespace str_er
