// line_decode_kernels.hip -- the line decoder on the device (gfx950): k_line_decode finds the cheapest string of every text line, blanks
// included, under the cost rows of its rows, the join / break costs of its gaps and the bigram table, with the decoder's DEL and INS
// moves, and backtracks it.  Integers only and no atomics: the output is the same bytes every time.  The rules are stated for the host
// in line_decode_rules.h; the contract is at str_er_line_decode in str_er.h.
//
// A line per wave, LD_LINES lines per workgroup; table, state vector and run step are k_word_decode's (word_decode_device.h): the table
// in LDS in rows of 68 bytes, state a of V in lane a with the states 64 and 65 in a second register of the lanes 0 and 1, a value with
// its state as a key, the min-plus product a lane a target and turned round for the target 64.  A gap is one more turned-round column,
// the one of the end of a word: X = min over a of V[a] + B[a][E] -- the break lands on E, which lives in lane 1, and that lane alone
// compares it with the join.  A line has up to 1024 rows, so the back pointers do not fit LDS: they go to a scratch table in device
// memory, 68 uint16 a row (the run step's word of the states 0 .. 65, then the gap's break | predecessor), which only this wave reads
// again.  Lane 0 backtracks into the tail of the line's slice of the label and source tables, then the wave moves the string to the
// front of the slice in chunks of 64 entries, ascending: the destination lies below the source.  The chain over the rows is serial per
// line: the kernel's time is the longest line's (profiles/line_decode.md).
#include <hip/hip_runtime.h>

#include "word_decode_device.h"
#include "line_decode_kernels.h"

namespace str_er {

namespace {

constexpr int      LD_THREADS = 64 * LD_LINES, LD_MAX_ROWS = 1024, LD_GAP = 66;
constexpr uint32_t LD_OFF = 255, LD_BREAK = 1u << 7;

__global__ void __launch_bounds__(LD_THREADS) k_line_decode(const uint8_t *__restrict__ bigram, int ins, int del, const uint8_t *__restrict__ costs,
                                                            const uint8_t *__restrict__ gaps, const int32_t *__restrict__ first_row, const int32_t *__restrict__ n_of,
                                                            const int32_t *__restrict__ row_map, int n_lines, uint16_t *bp, int32_t *__restrict__ dec, uint8_t *chars, uint16_t *src, int32_t *word_of_row)
{
    __shared__ __attribute__((aligned(16))) uint8_t  Bs[WD_STATES * WD_ROW];
    __shared__ __attribute__((aligned(16))) uint32_t vk[LD_LINES][WD_ROW], uk[LD_LINES][WD_ROW];
    __shared__ int32_t  rec[LD_LINES][8];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t = tid; t < WD_STATES * WD_ROW; t += LD_THREADS) {
        const int a = t / WD_ROW, b = t - a * WD_ROW;
        Bs[t] = b < WD_STATES ? bigram[a * WD_STATES + b] : (uint8_t)0;
    }
    __syncthreads();          // (the only barrier of the workgroup: from here on a wave is on its own)
    const int line = (int)blockIdx.x * LD_LINES + wave;
    if (line >= n_lines) return;
    const int    n = max(0, __builtin_amdgcn_readfirstlane(n_of[line]));
    const size_t first = (size_t)__builtin_amdgcn_readfirstlane(first_row[line]);
    uint8_t     *oc = chars + 3 * first;
    uint16_t    *os = src + 3 * first;
    int32_t     *wor = word_of_row + first;
    if (n > LD_MAX_ROWS) {          // not decoded
        for (int k = lane; k < 3 * n; k += 64) { oc[k] = (uint8_t)0xFF; os[k] = (uint16_t)0xFFFF; }
        for (int k = lane; k < n; k += 64) wor[k] = -1;
        if (lane < 6) dec[(size_t)line * 6 + lane] = lane == 0 ? -1 : 0;
        return;
    }
    const uint8_t *G = gaps + 2 * first;
    const int32_t *M = row_map ? row_map + first : nullptr;          // (the cost row of every row, where the rows of a line do not lie back to back)
    uint16_t      *bpl = bp + first * LD_BP_ROW;
    uint32_t      *vkw = vk[wave], *ukw = uk[wave];
    const uint8_t *bcol = Bs + lane;
    // V_0: the boundary at 0, every character at INF
    uint32_t key_lo = WD_INF << 7 | (uint32_t)lane;
    uint32_t key_hi = lane == 1 ? (uint32_t)WD_E : WD_INF << 7 | (uint32_t)(64 + (lane & 1));
    vkw[lane] = key_lo;
    if (lane < 2) vkw[64 + lane] = key_hi;
    for (int i = 1; i <= n; ++i) {
        uint16_t *st = bpl + (size_t)(i - 1) * LD_BP_ROW;
        if (i >= 2) {          // the gap in front of the row: every state joins, the boundary may come from a break
            const uint32_t J = (uint32_t)__builtin_amdgcn_readfirstlane((int)G[2 * (i - 1)]), K = (uint32_t)__builtin_amdgcn_readfirstlane((int)G[2 * (i - 1) + 1]);
            const uint32_t x = wd_column(Bs, lane, WD_E, key_lo, key_hi, 2);
            if (J == LD_OFF) {
                key_lo = WD_INF << 7 | (uint32_t)lane;
                key_hi = WD_INF << 7 | (uint32_t)(64 + (lane & 1));
            } else {
                key_lo += J << 7; key_hi += J << 7;
            }
            if (lane == 1) {
                uint32_t g = 0;
                if (K != LD_OFF && (x >> 7) + K < key_hi >> 7) { key_hi = ((x >> 7) + K) << 7 | (uint32_t)WD_E; g = LD_BREAK | (x & 127u); }
                st[LD_GAP] = (uint16_t)g;
            }
            vkw[lane] = key_lo;
            if (lane < 2) vkw[64 + lane] = key_hi;
        }
        wd_wave_sync();
        const uint8_t *row = costs + (M ? (size_t)__builtin_amdgcn_readfirstlane(M[i - 1]) : first + (size_t)(i - 1)) * WD_ALPHABET;
        const uint32_t cb = row[lane], c64 = row[64];
        // SUB
        const uint32_t s_lo = wd_product<WD_STATES>(vkw, key_lo, key_hi, bcol);
        const uint32_t s_64 = wd_column(Bs, lane, 64, key_lo, key_hi, 2);
        const uint32_t v_lo = key_lo >> 7, v_hi = key_hi >> 7;
        uint32_t u_lo = (s_lo >> 7) + cb, u_hi = lane == 0 ? (s_64 >> 7) + c64 : WD_INF;
        uint32_t e_lo = s_lo & 127u, e_hi = lane == 0 ? s_64 & 127u : 0u;
        if (del > 0) {
            if (v_lo + (uint32_t)del < u_lo) { u_lo = v_lo + (uint32_t)del; e_lo |= WD_DEL; }
            if (v_hi + (uint32_t)del < u_hi) { u_hi = v_hi + (uint32_t)del; e_hi |= WD_DEL; }
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
        st[lane] = (uint16_t)e_lo;
        if (lane < 2) { vkw[64 + lane] = key_hi; st[64 + lane] = (uint16_t)e_hi; }
    }
    const uint32_t end = wd_column(Bs, lane, WD_E, key_lo, key_hi, 2);
    wd_global_sync();
    if (lane == 0) {          // the backtrack: the string from its end, into the tail of the line's slice
        int state = (int)(end & 127u), at = 3 * n, n_sub = 0, n_del = 0, n_ins = 0, n_brk = 0;
        for (int i = n; i >= 1; --i) {
            const uint16_t *st = bpl + (size_t)(i - 1) * LD_BP_ROW;
            uint32_t        e = st[state];
            if (e & WD_INS) {
                oc[--at] = (uint8_t)state; os[at] = (uint16_t)((i - 1) | 0x8000);
                ++n_ins;
                state = (int)(e >> 9);
                e = st[state];
            }
            if (e & WD_DEL) { ++n_del; wor[i - 1] = -1; }
            else {
                oc[--at] = (uint8_t)state; os[at] = (uint16_t)(i - 1);
                wor[i - 1] = n_brk;          // (the breaks behind it: turned round below)
                ++n_sub;
                state = (int)(e & 127u);
            }
            if (i >= 2 && state == WD_E) {
                const uint32_t g = st[LD_GAP];
                if (g & LD_BREAK) {
                    oc[--at] = (uint8_t)WD_E; os[at] = (uint16_t)((i - 1) | 0x4000);
                    ++n_brk;
                    state = (int)(g & 127u);
                }
            }
        }
        rec[wave][0] = (int32_t)(end >> 7); rec[wave][1] = 3 * n - at; rec[wave][2] = n_brk;
        rec[wave][3] = n_sub; rec[wave][4] = n_del; rec[wave][5] = n_ins;
    }
    wd_global_sync();
    const int n_chars = rec[wave][1], n_brk = rec[wave][2], from = 3 * n - n_chars;          // (from >= 1 where n >= 1: a line emits at most 3n - 1)
    for (int c0 = 0; c0 < n_chars; c0 += 64) {          // ascending: chunk c is written below everything a later chunk reads
        const int k = c0 + lane;
        uint8_t   ch = 0;
        uint16_t  sv = 0;
        if (k < n_chars) { ch = oc[from + k]; sv = os[from + k]; }
        wd_global_sync();
        if (k < n_chars) { oc[k] = ch; os[k] = sv; }
    }
    for (int k = n_chars + lane; k < 3 * n; k += 64) { oc[k] = (uint8_t)0xFF; os[k] = (uint16_t)0xFFFF; }
    for (int k = lane; k < n; k += 64) {
        const int32_t v = wor[k];
        if (v >= 0) wor[k] = n_brk - v;
    }
    if (lane < 6) dec[(size_t)line * 6 + lane] = rec[wave][lane];
}

} // namespace

void launch_line_decode(hipStream_t s, const uint8_t *bigram, int ins, int del, const uint8_t *costs, const uint8_t *gaps, const int32_t *first_row, const int32_t *n_of,
                        const int32_t *row_map, int n_lines, uint16_t *bp, void *dec, uint8_t *chars, uint16_t *src, int32_t *word_of_row)
{
    if (n_lines <= 0) return;
    hipLaunchKernelGGL(k_line_decode, dim3((unsigned)((n_lines + LD_LINES - 1) / LD_LINES)), dim3(LD_THREADS), 0, s, bigram, ins, del, costs, gaps, first_row, n_of, row_map, n_lines,
                       bp, static_cast<int32_t *>(dec), chars, src, word_of_row);
}

} // namespace str_er
