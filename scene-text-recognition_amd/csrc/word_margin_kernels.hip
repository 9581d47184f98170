// word_margin_kernels.hip -- the margins of the open-vocabulary word decoder on the device (gfx950): k_word_margin makes the
// min-marginals of the decoder's recurrence -- for every run of a word and every reading of it the cost of the cheapest whole path that
// reads the run that way -- and from them the margin of every row and of the word.  Integers only and no atomics: the output is the
// same bytes every time.  The rules are stated for the host in word_margin_rules.h; the contract is at str_er_word_margin in str_er.h.
//
// A word per wave, WG_WORDS words per workgroup, behind k_word_decode, whose record, labels and sources say how the decoded string reads
// every row.  The table is staged as in k_word_decode (word_decode_device.h).  The wave runs the decoder's forward pass once more,
// without back pointers, and keeps V_0 .. V_{m-1} and S_1 .. S_m in LDS: every finite forward value is at most 32 * 255 * 2 = 16320, so
// 16 bits hold it and 0xFFFF stands for INF (an INF entry never wins, so what was added to it is not needed).  Then the backward pass:
// its min-plus product is the transpose of the forward one -- lane b reads row b of the staged table, 17 words from an address of
// stride 17 words, which is odd: no two lanes on one bank -- against a vector every lane reads at one address (a broadcast).  The
// states 64 and 65 live in the second register of the lanes 0 and 1; their entries are computed the turned-round way, a lane per
// column and the wave minimum, and so is the marginal of dropping the row.  The margin of a row is the wave minimum of the keys
// marginal << 7 | reading with the decoded reading left out: the smallest reading among equals for free.  Row i - 1's results wait in
// lane i - 1 and go out in one write at the end.  The loops over the runs are run-time loops and no array lives in registers.
//
// LDS per workgroup: 4488 bytes of table, 2 x 1088 of vectors, 2 x 16896 of forward values, 128 of readings: 40592 bytes with the
// padding between them, three workgroups (twelve waves) a CU by LDS.
#include <hip/hip_runtime.h>

#include "word_margin_device.h"
#include "word_margin_kernels.h"

namespace str_er {

namespace {

constexpr int      WG_THREADS = 64 * WG_WORDS, WG_MARGINALS = WD_STATES;
constexpr uint32_t WG_NONE16 = 0xFFFFu;

__device__ __forceinline__ uint32_t wg_load16(uint16_t v) { return v == WG_NONE16 ? WD_INF : (uint32_t)v; }
__device__ __forceinline__ uint16_t wg_store16(uint32_t v) { return (uint16_t)min(v, WG_NONE16); }

__global__ void __launch_bounds__(WG_THREADS) k_word_margin(const uint8_t *__restrict__ bigram, int ins, int del, const uint8_t *__restrict__ costs,
                                                            const int32_t *__restrict__ first_run, const int32_t *__restrict__ n_of, int n_words,
                                                            const int32_t *__restrict__ dec, const uint8_t *__restrict__ chars, const uint8_t *__restrict__ src,
                                                            int32_t *__restrict__ margins, int32_t *__restrict__ row_margin, uint8_t *__restrict__ row_read,
                                                            uint8_t *__restrict__ row_alt, int32_t *__restrict__ marginals)
{
    __shared__ __attribute__((aligned(16))) uint32_t Bw[WD_STATES * WG_ROW_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t vk[WG_WORDS][WD_ROW], uk[WG_WORDS][WD_ROW];
    __shared__ uint16_t sV[WG_WORDS][WD_MAX_RUNS][WD_STATES], sS[WG_WORDS][WD_MAX_RUNS][WD_STATES];
    __shared__ uint8_t  xr[WG_WORDS][WD_MAX_RUNS];
    uint8_t  *Bs = reinterpret_cast<uint8_t *>(Bw);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t = tid; t < WD_STATES * WD_ROW; t += WG_THREADS) {
        const int a = t / WD_ROW, b = t - a * WD_ROW;
        Bs[t] = b < WD_STATES ? bigram[a * WD_STATES + b] : (uint8_t)0;
    }
    __syncthreads();          // (the only barrier of the workgroup: from here on a wave is on its own)
    const int w = (int)blockIdx.x * WG_WORDS + wave;
    if (w >= n_words) return;
    const int m = __builtin_amdgcn_readfirstlane(n_of[w]);
    int32_t  *mg = marginals ? marginals + (size_t)w * (WD_MAX_RUNS * WG_MARGINALS) : nullptr;
    int32_t   my_margin = -1;                      // of row `lane`, for lane < m
    uint32_t  my_read = 0xFFu, my_alt = 0xFFu;
    int       done = 0;                            // rows whose marginals are written
    if (m >= 1 && m <= WD_MAX_RUNS) {
        const uint8_t  *C = costs + (size_t)__builtin_amdgcn_readfirstlane(first_run[w]) * WD_ALPHABET;
        uint32_t       *vkw = vk[wave], *ukw = uk[wave];
        const uint8_t  *bcol = Bs + lane;
        const uint32_t *brow = Bw + lane * WG_ROW_WORDS;
        // the reading of every row: the label of the character of the decoded string whose source is the row, or 65
        const int n_chars = __builtin_amdgcn_readfirstlane(dec[(size_t)w * 6 + 2]);
        if (lane < WD_MAX_RUNS) xr[wave][lane] = (uint8_t)WD_E;
        wd_wave_sync();
        if (lane < n_chars) {
            const uint32_t from = src[(size_t)w * 64 + lane];
            if (from < (uint32_t)m) xr[wave][from] = chars[(size_t)w * 64 + lane];          // (bit 7 set: inserted, no row)
        }
        // the forward pass of k_word_decode: V_0 is the boundary at 0, every character at INF
        uint32_t key_lo = WD_INF << 7 | (uint32_t)lane;
        uint32_t key_hi = lane == 1 ? (uint32_t)WD_E : WD_INF << 7 | (uint32_t)(64 + (lane & 1));
        vkw[lane] = key_lo;
        if (lane < 2) vkw[64 + lane] = key_hi;
        for (int i = 1; i <= m; ++i) {
            wd_wave_sync();
            const uint8_t *row = C + (size_t)(i - 1) * WD_ALPHABET;
            const uint32_t cb = row[lane], c64 = row[64];
            const uint32_t s_lo = wd_product<WD_STATES>(vkw, key_lo, key_hi, bcol);
            const uint32_t s_64 = wd_column(Bs, lane, 64, key_lo, key_hi, 2);
            const uint32_t v_lo = key_lo >> 7, v_hi = key_hi >> 7;
            uint32_t u_lo = (s_lo >> 7) + cb, u_hi = lane == 0 ? (s_64 >> 7) + c64 : WD_INF;
            sV[wave][i - 1][lane] = wg_store16(v_lo); sS[wave][i - 1][lane] = wg_store16(u_lo);
            if (lane < 2) sV[wave][i - 1][64 + lane] = wg_store16(v_hi);
            if (lane == 0) sS[wave][i - 1][64] = wg_store16(u_hi);
            if (del > 0) {
                u_lo = min(u_lo, v_lo + (uint32_t)del);
                u_hi = min(u_hi, v_hi + (uint32_t)del);
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
        }
        const uint32_t cost = wd_column(Bs, lane, WD_E, key_lo, key_hi, 2) >> 7;
        // the backward pass: G_m[a] = B[a][E]; G of the states 64 and 65 in g_hi of the lanes 0 and 1
        uint32_t g_lo = Bs[lane * WD_ROW + WD_E], g_hi = lane < 2 ? (uint32_t)Bs[(64 + lane) * WD_ROW + WD_E] : WD_INF;
        for (int i = m; i >= 1; --i) {
            const uint8_t *row = C + (size_t)(i - 1) * WD_ALPHABET;
            const uint32_t cb = row[lane], c64 = row[64];
            // GU: a character inserted behind the row's
            uint32_t gu_lo = g_lo, gu_hi = g_hi;
            if (ins > 0) {
                wd_wave_sync();
                vkw[lane] = g_lo;
                if (lane == 0) vkw[64] = g_hi;
                wd_wave_sync();
                const uint32_t t_lo = wg_product_t(vkw, brow), t_64 = wg_row(Bs, lane, 64, g_lo, g_hi);
                gu_lo = min(g_lo, t_lo + (uint32_t)ins);
                if (lane == 0) gu_hi = min(g_hi, t_64 + (uint32_t)ins);
            }
            // the marginals: the row read as the lane's label (m_64: as 64, in lane 0) or dropped (m_65, in every lane)
            const uint32_t m_lo = wg_load16(sS[wave][i - 1][lane]) + gu_lo, m_64 = wg_load16(sS[wave][i - 1][64]) + gu_hi;
            uint32_t       m_65 = WD_INF;
            if (del > 0) {
                uint32_t t = wg_load16(sV[wave][i - 1][lane]) + (uint32_t)del + gu_lo;
                if (lane < 2) t = min(t, wg_load16(sV[wave][i - 1][64 + lane]) + (uint32_t)del + gu_hi);
                m_65 = wd_wave_min(t);
            }
            const uint32_t x = xr[wave][i - 1];
            uint32_t       key = (uint32_t)lane != x && m_lo < WD_INF ? m_lo << 7 | (uint32_t)lane : ~0u;
            if (lane == 0 && x != 64u && m_64 < WD_INF) key = min(key, m_64 << 7 | 64u);
            if (lane == 1 && x != 65u && m_65 < WD_INF) key = min(key, m_65 << 7 | 65u);
            key = wd_wave_min(key);
            if (lane == i - 1) { my_margin = (int32_t)(key >> 7) - (int32_t)cost; my_read = x; my_alt = key & 127u; }
            if (mg) {
                int32_t *out = mg + (i - 1) * WG_MARGINALS;
                out[lane] = m_lo < WD_INF ? (int32_t)m_lo : -1;
                if (lane == 0) out[64] = m_64 < WD_INF ? (int32_t)m_64 : -1;
                if (lane == 1) out[65] = m_65 < WD_INF ? (int32_t)m_65 : -1;
            }
            // G_{i-1}[a] = min over b < 65 of B[a][b] + C_i[b] + GU_i[b], and DEL + GU_i[a]
            wd_wave_sync();
            const uint32_t h_lo = cb + gu_lo, h_64 = c64 + gu_hi;          // (h_64 counts in lane 0 alone)
            ukw[lane] = h_lo;
            if (lane == 0) ukw[64] = h_64;
            wd_wave_sync();
            const uint32_t n_lo = wg_product_t(ukw, brow), n_64 = wg_row(Bs, lane, 64, h_lo, h_64), n_65 = wg_row(Bs, lane, WD_E, h_lo, h_64);
            g_lo = n_lo;
            g_hi = lane == 0 ? n_64 : lane == 1 ? n_65 : WD_INF;
            if (del > 0) {
                g_lo = min(g_lo, (uint32_t)del + gu_lo);
                if (lane < 2) g_hi = min(g_hi, (uint32_t)del + gu_hi);
            }
        }
        done = m;
    }
    // the word: the smallest margin at the smallest row (a margin is below 2^15)
    uint32_t wkey = lane < done ? (uint32_t)my_margin << 5 | (uint32_t)lane : ~0u;
    wkey = wd_wave_min(wkey);
    const int      wrow = done > 0 ? (int)(wkey & 31u) : 0;
    const uint32_t wread = (uint32_t)__shfl((int)my_read, wrow, 64), walt = (uint32_t)__shfl((int)my_alt, wrow, 64);
    if (lane < 4) {
        const int32_t v = lane == 0 ? (int32_t)(wkey >> 5) : lane == 1 ? wrow : lane == 2 ? (int32_t)wread : (int32_t)walt;
        margins[(size_t)w * 4 + lane] = done > 0 ? v : -1;
    }
    if (lane < WD_MAX_RUNS) {
        row_margin[(size_t)w * WD_MAX_RUNS + lane] = my_margin;
        row_read[(size_t)w * WD_MAX_RUNS + lane] = (uint8_t)my_read;
        row_alt[(size_t)w * WD_MAX_RUNS + lane] = (uint8_t)my_alt;
    }
    if (mg)
        for (int t = done * WG_MARGINALS + lane; t < WD_MAX_RUNS * WG_MARGINALS; t += 64) mg[t] = -1;
}

} // namespace

void launch_word_margin(hipStream_t s, const uint8_t *bigram, int ins, int del, const uint8_t *costs, const int32_t *first_run, const int32_t *n_of, int n_words,
                        const void *dec, const uint8_t *chars, const uint8_t *src, void *margins, int32_t *row_margin, uint8_t *row_read, uint8_t *row_alt,
                        int32_t *marginals)
{
    if (n_words <= 0) return;
    hipLaunchKernelGGL(k_word_margin, dim3((unsigned)((n_words + WG_WORDS - 1) / WG_WORDS)), dim3(WG_THREADS), 0, s, bigram, ins, del, costs, first_run, n_of, n_words,
                       static_cast<const int32_t *>(dec), chars, src, static_cast<int32_t *>(margins), row_margin, row_read, row_alt, marginals);
}

} // namespace str_er
