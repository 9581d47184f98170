// line_margin_kernels.hip -- the margins of the line decoder on the device (gfx950): k_line_margin makes the min-marginals of the
// decoder's recurrence -- for every row of a line and every reading of it, and for every gap and either move at it, the cost of the
// cheapest whole path that does just that -- and from them the margin of every row, of every gap and of the line.  Integers only and no
// atomics: the output is the same bytes every time.  The rules are stated for the host in line_margin_rules.h; the contract is at
// str_er_line_margin in str_er.h.
//
// A line per wave, LD_LINES lines per workgroup, behind k_line_decode, whose record, labels and sources say how the decoded string
// reads every row and decides every gap: the wave scatters them into row_read and gap_move first, and reads them back row by row.  The
// table is staged as in k_word_margin, the state vector lives as in k_line_decode.  The wave runs the decoder's forward pass once more,
// without back pointers, and writes V_{i-1}, X_i and S_i of every row into the line's slice of a scratch table in device memory, 136
// uint32 a row: a line has up to 1024 rows and its values reach 2^25, so neither LDS nor 16 bits hold them.  Only this wave reads the
// slice again (wd_global_sync, as in k_line_decode), and every lane reads what it wrote itself but X_i.  Then the backward pass with
// the transposed products of word_margin_device.h: GU from G, the marginals of the row, H from GU, the two marginals of the gap --
// the join as a wave minimum over V_{i-1} + J + H, the break from the stored X_i and H[E], which lane 1 holds -- and G of the row
// before.  A row's results go out as the pass reaches it; the line's record comes from two running keys, margin << 10 | row, which
// are the same in every lane.  The loops over the rows are run-time loops and no array lives in registers.  The chain over the rows is
// serial per line, twice: the kernel's time is the longest line's (profiles/line_margin.md).
#include <hip/hip_runtime.h>

#include "word_margin_device.h"
#include "line_margin_kernels.h"

namespace str_er {

namespace {

constexpr int      LM_THREADS = 64 * LD_LINES, LM_MAX_ROWS = 1024, LM_X = 66, LM_S = 68, LM_JOIN = 66, LM_BREAK = 67;
constexpr uint32_t LM_OFF = 255;

__device__ __forceinline__ int32_t lm_out(uint32_t v) { return v < WD_INF ? (int32_t)v : -1; }

__global__ void __launch_bounds__(LM_THREADS) k_line_margin(const uint8_t *__restrict__ bigram, int ins, int del, const uint8_t *__restrict__ costs,
                                                            const uint8_t *__restrict__ gaps, const int32_t *__restrict__ first_row, const int32_t *__restrict__ n_of,
                                                            const int32_t *__restrict__ row_map, int n_lines, const int32_t *__restrict__ dec,
                                                            const uint8_t *__restrict__ chars, const uint16_t *__restrict__ src, uint32_t *fw, int32_t *__restrict__ margins,
                                                            int32_t *__restrict__ row_margin, uint8_t *row_read, uint8_t *__restrict__ row_alt,
                                                            int32_t *__restrict__ gap_margin, uint8_t *gap_move, int32_t *__restrict__ marginals)
{
    __shared__ __attribute__((aligned(16))) uint32_t Bw[WD_STATES * WG_ROW_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t vk[LD_LINES][WD_ROW], uk[LD_LINES][WD_ROW];
    uint8_t  *Bs = reinterpret_cast<uint8_t *>(Bw);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t = tid; t < WD_STATES * WD_ROW; t += LM_THREADS) {
        const int a = t / WD_ROW, b = t - a * WD_ROW;
        Bs[t] = b < WD_STATES ? bigram[a * WD_STATES + b] : (uint8_t)0;
    }
    __syncthreads();          // (the only barrier of the workgroup: from here on a wave is on its own)
    const int line = (int)blockIdx.x * LD_LINES + wave;
    if (line >= n_lines) return;
    const int    n = max(0, __builtin_amdgcn_readfirstlane(n_of[line]));
    const size_t first = (size_t)__builtin_amdgcn_readfirstlane(first_row[line]);
    int32_t     *rm = row_margin + first, *gm = gap_margin + first, *rec = margins + (size_t)line * 8;
    uint8_t     *rr = row_read + first, *ra = row_alt + first, *gv = gap_move + first;
    int32_t     *mg = marginals ? marginals + first * LM_MARGINALS : nullptr;
    if (n == 0 || n > LM_MAX_ROWS) {          // no rows, or not decoded
        for (int k = lane; k < n; k += 64) { rm[k] = -1; gm[k] = -1; rr[k] = (uint8_t)0xFF; ra[k] = (uint8_t)0xFF; gv[k] = (uint8_t)0xFF; }
        if (mg)
            for (int k = lane; k < n * LM_MARGINALS; k += 64) mg[k] = -1;
        if (lane < 8) rec[lane] = -1;
        return;
    }
    const uint8_t  *G = gaps + 2 * first;
    const int32_t  *M = row_map ? row_map + first : nullptr;          // (the cost row of every row, where the rows of a line do not lie back to back)
    uint32_t       *fwl = fw + first * LM_FW_ROW;
    uint32_t       *vkw = vk[wave], *ukw = uk[wave];
    const uint8_t  *bcol = Bs + lane;
    const uint32_t *brow = Bw + lane * WG_ROW_WORDS;
    // the reading of every row and the move of every gap: a row the string does not name is dropped, a gap it does not name a join
    for (int k = lane; k < n; k += 64) { rr[k] = (uint8_t)WD_E; gv[k] = k == 0 ? (uint8_t)0xFF : (uint8_t)0; }
    wd_global_sync();
    {
        const int       n_chars = min(3 * n, __builtin_amdgcn_readfirstlane(dec[(size_t)line * 6 + 1]));
        const uint8_t  *oc = chars + 3 * first;
        const uint16_t *os = src + 3 * first;
        for (int k = lane; k < n_chars; k += 64) {
            const uint32_t sv = os[k], at = sv & 0x3FFFu, flags = sv & 0xC000u;
            if (at >= (uint32_t)n) continue;
            if (flags == 0u) rr[at] = oc[k];
            else if (flags == 0x4000u && at >= 1u) gv[at] = (uint8_t)1;
        }
    }
    // the forward pass of k_line_decode: V_0 is the boundary at 0, every character at INF
    uint32_t key_lo = WD_INF << 7 | (uint32_t)lane;
    uint32_t key_hi = lane == 1 ? (uint32_t)WD_E : WD_INF << 7 | (uint32_t)(64 + (lane & 1));
    vkw[lane] = key_lo;
    if (lane < 2) vkw[64 + lane] = key_hi;
    for (int i = 1; i <= n; ++i) {
        uint32_t *fr = fwl + (size_t)(i - 1) * LM_FW_ROW;
        fr[lane] = key_lo >> 7;
        if (lane < 2) fr[64 + lane] = key_hi >> 7;
        uint32_t xs = WD_INF;
        if (i >= 2) {          // the gap in front of the row: every state joins, the boundary may come from a break
            const uint32_t J = (uint32_t)__builtin_amdgcn_readfirstlane((int)G[2 * (i - 1)]), K = (uint32_t)__builtin_amdgcn_readfirstlane((int)G[2 * (i - 1) + 1]);
            const uint32_t x = wd_column(Bs, lane, WD_E, key_lo, key_hi, 2);
            if (J == LM_OFF) {
                key_lo = WD_INF << 7 | (uint32_t)lane;
                key_hi = WD_INF << 7 | (uint32_t)(64 + (lane & 1));
            } else {
                key_lo += J << 7; key_hi += J << 7;
            }
            if (K != LM_OFF) {
                xs = (x >> 7) + K;
                if (lane == 1 && xs < key_hi >> 7) key_hi = xs << 7 | (uint32_t)WD_E;
            }
            vkw[lane] = key_lo;
            if (lane < 2) vkw[64 + lane] = key_hi;
        }
        if (lane == 0) fr[LM_X] = xs;
        wd_wave_sync();
        const uint8_t *row = costs + (M ? (size_t)__builtin_amdgcn_readfirstlane(M[i - 1]) : first + (size_t)(i - 1)) * WD_ALPHABET;
        const uint32_t cb = row[lane], c64 = row[64];
        const uint32_t s_lo = wd_product<WD_STATES>(vkw, key_lo, key_hi, bcol);
        const uint32_t s_64 = wd_column(Bs, lane, 64, key_lo, key_hi, 2);
        const uint32_t v_lo = key_lo >> 7, v_hi = key_hi >> 7;
        uint32_t u_lo = (s_lo >> 7) + cb, u_hi = lane == 0 ? (s_64 >> 7) + c64 : WD_INF;
        fr[LM_S + lane] = u_lo;
        if (lane == 0) fr[LM_S + 64] = u_hi;
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
        if (lane < 2) { vkw[64 + lane] = key_hi; }
    }
    const uint32_t cost = wd_column(Bs, lane, WD_E, key_lo, key_hi, 2) >> 7;
    wd_global_sync();
    // the backward pass: G_n[a] = B[a][E]; G of the states 64 and 65 in g_hi of the lanes 0 and 1
    const uint32_t be_lo = Bs[lane * WD_ROW + WD_E], be_hi = lane < 2 ? (uint32_t)Bs[(64 + lane) * WD_ROW + WD_E] : WD_INF;
    uint32_t g_lo = be_lo, g_hi = be_hi;
    uint32_t rkey = ~0u, r_read = 0u, r_alt = 0u, gkey = ~0u, g_move = 0u;          // (the same in every lane)
    for (int i = n; i >= 1; --i) {
        const uint32_t *fr = fwl + (size_t)(i - 1) * LM_FW_ROW;
        const uint8_t  *row = costs + (M ? (size_t)__builtin_amdgcn_readfirstlane(M[i - 1]) : first + (size_t)(i - 1)) * WD_ALPHABET;
        const uint32_t  cb = row[lane], c64 = row[64];
        const uint32_t  v_lo = fr[lane], v_hi = lane < 2 ? fr[64 + lane] : WD_INF, xs = fr[LM_X], s_lo = fr[LM_S + lane], s_64 = fr[LM_S + 64];
        const uint32_t  J = i >= 2 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)G[2 * (i - 1)]) : 0u;
        const uint32_t  K = i >= 2 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)G[2 * (i - 1) + 1]) : LM_OFF;
        const uint32_t  x = (uint32_t)__builtin_amdgcn_readfirstlane((int)rr[i - 1]);
        const uint32_t  d = i >= 2 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)gv[i - 1]) : 0u;
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
        // the marginals of the row: read as the lane's label (m_64: as 64, in lane 0) or dropped (m_65, in every lane), from W_i
        const uint32_t m_lo = s_lo + gu_lo, m_64 = s_64 + gu_hi;
        uint32_t       m_65 = WD_INF;
        if (del > 0) {
            uint32_t w_lo = i == 1 ? v_lo : J == LM_OFF ? WD_INF : v_lo + J, w_hi = i == 1 ? v_hi : J == LM_OFF ? WD_INF : v_hi + J;
            if (lane == 1 && K != LM_OFF) w_hi = min(w_hi, xs);
            uint32_t t = w_lo + (uint32_t)del + gu_lo;
            if (lane < 2) t = min(t, w_hi + (uint32_t)del + gu_hi);
            m_65 = wd_wave_min(t);
        }
        uint32_t key = (uint32_t)lane != x && m_lo < WD_INF ? m_lo << 7 | (uint32_t)lane : ~0u;
        if (lane == 0 && x != 64u && m_64 < WD_INF) key = min(key, m_64 << 7 | 64u);
        if (lane == 1 && x != 65u && m_65 < WD_INF) key = min(key, m_65 << 7 | 65u);
        key = wd_wave_min(key);
        const uint32_t margin = (key >> 7) - cost, alt = key & 127u;
        if (lane == 0) { rm[i - 1] = (int32_t)margin; ra[i - 1] = (uint8_t)alt; }
        if ((margin << 10 | (uint32_t)(i - 1)) < rkey) { rkey = margin << 10 | (uint32_t)(i - 1); r_read = x; r_alt = alt; }
        // H_i[a] = min over b < 65 of B[a][b] + C_i[b] + GU_i[b], and DEL + GU_i[a]
        wd_wave_sync();
        const uint32_t c_lo = cb + gu_lo, c_64 = c64 + gu_hi;          // (c_64 counts in lane 0 alone)
        ukw[lane] = c_lo;
        if (lane == 0) ukw[64] = c_64;
        wd_wave_sync();
        const uint32_t n_lo = wg_product_t(ukw, brow), n_64 = wg_row(Bs, lane, 64, c_lo, c_64), n_65 = wg_row(Bs, lane, WD_E, c_lo, c_64);
        uint32_t h_lo = n_lo, h_hi = lane == 0 ? n_64 : lane == 1 ? n_65 : WD_INF;
        if (del > 0) {
            h_lo = min(h_lo, (uint32_t)del + gu_lo);
            if (lane < 2) h_hi = min(h_hi, (uint32_t)del + gu_hi);
        }
        uint32_t m_j = WD_INF, m_k = WD_INF;
        if (i >= 2) {          // the gap in front of the row: its two marginals, its margin, and G of the row before
            const uint32_t h_e = (uint32_t)__builtin_amdgcn_readlane((int)h_hi, 1);
            if (J != LM_OFF) {
                uint32_t t = v_lo + J + h_lo;
                if (lane < 2) t = min(t, v_hi + J + h_hi);
                m_j = wd_wave_min(t);
            }
            if (K != LM_OFF) m_k = xs + h_e;
            const uint32_t other = d ? m_j : m_k;
            if (lane == 0) gm[i - 1] = other < WD_INF ? (int32_t)(other - cost) : -1;
            if (other < WD_INF && ((other - cost) << 10 | (uint32_t)(i - 1)) < gkey) { gkey = (other - cost) << 10 | (uint32_t)(i - 1); g_move = d; }
            // (far: only for a gap with both moves off, which no caller sends -- gaps_ok refuses it and gap_costs never makes it; it is
            // the result then, nothing is added to it)
            const uint32_t far = WD_INF << 5;
            g_lo = min(J != LM_OFF ? J + h_lo : far, K != LM_OFF ? be_lo + K + h_e : far);
            g_hi = lane < 2 ? min(J != LM_OFF ? J + h_hi : far, K != LM_OFF ? be_hi + K + h_e : far) : WD_INF;
        }
        if (mg) {
            int32_t *out = mg + (size_t)(i - 1) * LM_MARGINALS;
            out[lane] = lm_out(m_lo);
            if (lane == 0) out[64] = lm_out(m_64);
            if (lane == 1) out[65] = lm_out(m_65);
            if (lane == 2) out[LM_JOIN] = lm_out(m_j);
            if (lane == 3) out[LM_BREAK] = lm_out(m_k);
        }
    }
    // the line: the smallest row margin at the smallest row, the smallest gap margin at the smallest gap
    if (lane < 8) {
        const bool    gap = gkey != ~0u;
        const int32_t rmin = (int32_t)(rkey >> 10), gmin = gap ? (int32_t)(gkey >> 10) : -1;
        const int32_t v = lane == 0 ? (gap && gmin < rmin ? gmin : rmin) : lane == 1 ? rmin : lane == 2 ? (int32_t)(rkey & 1023u) : lane == 3 ? (int32_t)r_read
                        : lane == 4 ? (int32_t)r_alt : lane == 5 ? gmin : lane == 6 ? (gap ? (int32_t)(gkey & 1023u) : -1) : (gap ? (int32_t)g_move : -1);
        rec[lane] = v;
    }
}

} // namespace

void launch_line_margin(hipStream_t s, const uint8_t *bigram, int ins, int del, const uint8_t *costs, const uint8_t *gaps, const int32_t *first_row, const int32_t *n_of,
                        const int32_t *row_map, int n_lines, const void *dec, const uint8_t *chars, const uint16_t *src, uint32_t *fw, void *margins, int32_t *row_margin,
                        uint8_t *row_read, uint8_t *row_alt, int32_t *gap_margin, uint8_t *gap_move, int32_t *marginals)
{
    if (n_lines <= 0) return;
    hipLaunchKernelGGL(k_line_margin, dim3((unsigned)((n_lines + LD_LINES - 1) / LD_LINES)), dim3(LM_THREADS), 0, s, bigram, ins, del, costs, gaps, first_row, n_of, row_map,
                       n_lines, static_cast<const int32_t *>(dec), chars, src, fw, static_cast<int32_t *>(margins), row_margin, row_read, row_alt, gap_margin, gap_move, marginals);
}

} // namespace str_er
