// word_decode_kernels.hip -- the open-vocabulary word decoder on the device (gfx950): k_word_decode finds the cheapest character string
// of every word under the cost rows of its glyph runs plus a bigram table, with the optional DEL and INS moves, and backtracks it.
// Integers only and no atomics: the output is the same bytes every time.  The rules are stated for the host in word_decode_rules.h;
// the contract is at str_er_word_decode in str_er.h.
//
// A word per wave, WD_WORDS words per workgroup.  The table is staged once per workgroup in LDS, row-major with rows of 68 bytes: lane b
// reads the bytes B[a][b] of one row a at a time (64 consecutive bytes of an aligned row: 16 words, no two lanes on one bank with
// different words), and the column reads B[l][64], B[l][65] of the tail stride over 17 words, which is odd: no conflict either.
// State a of V lives in lane a for a < 64; the states 64 (the character ')') and 65 (the boundary) live in a second register of the
// lanes 0 and 1.  The min-plus product for the targets 0 .. 63 is a loop over the 66 predecessors, a lane a target; for the target 64 it
// is turned round: every lane adds its own state's value to B[a][64] and the wave takes the minimum.  A value travels with its state
// as a key (value << 7 | state): the minimum of the keys is the minimum value at the smallest state, which is the tie rule.
// The predecessors' keys reach the lanes through LDS (one address for the whole wave: a broadcast); WD_READLANE takes them across the
// lanes with v_readlane instead (measured: profiles/word_decode.md).  The loop over the runs is a run-time loop and no array lives in
// registers: there is nothing to bucket by the run count.
#include <hip/hip_runtime.h>

#include "word_decode_device.h"
#include "word_decode_kernels.h"

namespace str_er {

namespace {

constexpr int      WD_THREADS = 64 * WD_WORDS;

__global__ void __launch_bounds__(WD_THREADS) k_word_decode(const uint8_t *__restrict__ bigram, int ins, int del, const uint8_t *__restrict__ costs,
                                                            const int32_t *__restrict__ first_run, const int32_t *__restrict__ n_of, int n_words,
                                                            int32_t *__restrict__ dec, uint8_t *__restrict__ chars, uint8_t *__restrict__ src)
{
    __shared__ __attribute__((aligned(16))) uint8_t  Bs[WD_STATES * WD_ROW];
    __shared__ __attribute__((aligned(16))) uint32_t vk[WD_WORDS][WD_ROW], uk[WD_WORDS][WD_ROW];
    __shared__ uint16_t bp[WD_WORDS][WD_MAX_RUNS][WD_STATES];
    __shared__ uint8_t  out_c[WD_WORDS][64], out_s[WD_WORDS][64];
    __shared__ int32_t  rec[WD_WORDS][8];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t = tid; t < WD_STATES * WD_ROW; t += WD_THREADS) {
        const int a = t / WD_ROW, b = t - a * WD_ROW;
        Bs[t] = b < WD_STATES ? bigram[a * WD_STATES + b] : (uint8_t)0;
    }
    __syncthreads();          // (the only barrier of the workgroup: from here on a wave is on its own)
    const int w = (int)blockIdx.x * WD_WORDS + wave;
    if (w >= n_words) return;
    const int      m = max(0, __builtin_amdgcn_readfirstlane(n_of[w]));
    const uint8_t *C = costs + (size_t)__builtin_amdgcn_readfirstlane(first_run[w]) * WD_ALPHABET;
    uint32_t      *vkw = vk[wave], *ukw = uk[wave];
    const uint8_t *bcol = Bs + lane;
    int            prev = WD_E, n_chars = 0;
    int32_t        rc = 0;
    if (m > WD_MAX_RUNS) {          // not decoded: the plain reading's cost alone
        for (int i = 0; i < m; ++i) wd_read_step(Bs, lane, C[(size_t)i * WD_ALPHABET + lane], C[(size_t)i * WD_ALPHABET + 64], prev, rc);
        if (lane == 0) {
            rec[wave][0] = -1; rec[wave][1] = rc + (int32_t)Bs[prev * WD_ROW + WD_E];
            rec[wave][2] = rec[wave][3] = rec[wave][4] = rec[wave][5] = 0;
        }
    } else {
        // V_0: the boundary at 0, every character at INF
        uint32_t key_lo = WD_INF << 7 | (uint32_t)lane;
        uint32_t key_hi = lane == 1 ? (uint32_t)WD_E : WD_INF << 7 | (uint32_t)(64 + (lane & 1));
        vkw[lane] = key_lo;
        if (lane < 2) vkw[64 + lane] = key_hi;
        for (int i = 1; i <= m; ++i) {
            wd_wave_sync();
            const uint8_t *row = C + (size_t)(i - 1) * WD_ALPHABET;
            const uint32_t cb = row[lane], c64 = row[64];
            wd_read_step(Bs, lane, cb, c64, prev, rc);
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
            bp[wave][i - 1][lane] = (uint16_t)e_lo;
            if (lane < 2) { vkw[64 + lane] = key_hi; bp[wave][i - 1][64 + lane] = (uint16_t)e_hi; }
        }
        const uint32_t end = wd_column(Bs, lane, WD_E, key_lo, key_hi, 2);
        wd_wave_sync();
        if (lane == 0) {          // the backtrack: the string from its end, into the tail of out_c / out_s
            int state = (int)(end & 127u), at = 64, n_sub = 0, n_del = 0, n_ins = 0;
            for (int i = m; i >= 1; --i) {
                const uint16_t *st = bp[wave][i - 1];
                uint32_t        e = st[state];
                if (e & WD_INS) {
                    out_c[wave][--at] = (uint8_t)state; out_s[wave][at] = (uint8_t)((i - 1) | 0x80);
                    ++n_ins;
                    state = (int)(e >> 9);
                    e = st[state];
                }
                if (e & WD_DEL) ++n_del;
                else {
                    out_c[wave][--at] = (uint8_t)state; out_s[wave][at] = (uint8_t)(i - 1);
                    ++n_sub;
                    state = (int)(e & 127u);
                }
            }
            rec[wave][0] = (int32_t)(end >> 7); rec[wave][1] = rc + (int32_t)Bs[prev * WD_ROW + WD_E];
            rec[wave][2] = 64 - at; rec[wave][3] = n_sub; rec[wave][4] = n_del; rec[wave][5] = n_ins;
        }
    }
    wd_wave_sync();
    n_chars = rec[wave][2];
    const int from = 64 - n_chars + lane;          // (n_chars <= 64: the string sits at the end of out_c)
    chars[(size_t)w * 64 + lane] = lane < n_chars ? out_c[wave][from] : (uint8_t)0xFF;
    src[(size_t)w * 64 + lane] = lane < n_chars ? out_s[wave][from] : (uint8_t)0xFF;
    if (lane < 6) dec[(size_t)w * 6 + lane] = rec[wave][lane];
}

} // namespace

void launch_word_decode(hipStream_t s, const uint8_t *bigram, int ins, int del, const uint8_t *costs, const int32_t *first_run, const int32_t *n_of, int n_words,
                        void *dec, uint8_t *chars, uint8_t *src)
{
    if (n_words <= 0) return;
    hipLaunchKernelGGL(k_word_decode, dim3((unsigned)((n_words + WD_WORDS - 1) / WD_WORDS)), dim3(WD_THREADS), 0, s, bigram, ins, del, costs, first_run, n_of,
                       n_words, static_cast<int32_t *>(dec), chars, src);
}

} // namespace str_er
