// word_margin_device.h -- INTERNAL: the device pieces the margin kernels of the bigram decoders share (word_margin_kernels.hip:
// k_word_margin, line_margin_kernels.hip: k_line_margin) on top of word_decode_device.h: the min-plus product of the backward pass,
// which is the transpose of the forward one -- lane b reads row b of the staged table, 17 words from an address of stride 17 words,
// which is odd: no two lanes on one bank -- against a vector every lane reads at one address (a broadcast), and its turned-round form
// for the rows 64 and 65 of the table.  The table is staged as words (WG_ROW_WORDS a row) so that a row is read four bytes at a time.
#pragma once
#include "word_decode_device.h"

namespace str_er {

namespace {

constexpr int WG_ROW_WORDS = WD_ROW / 4;

// min over c in [0, 65) of B[lane][c] + vec[c]; brow = the words of the table's row of the lane.  Fully unrolled: every offset is an immediate.
__device__ __forceinline__ uint32_t wg_product_t(const uint32_t *vec, const uint32_t *brow)
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
__device__ __forceinline__ uint32_t wg_row(const uint8_t *Bs, int lane, int a, uint32_t v_lo, uint32_t v_64)
{
    uint32_t t = v_lo + (uint32_t)Bs[a * WD_ROW + lane];
    if (lane == 0) t = min(t, v_64 + (uint32_t)Bs[a * WD_ROW + 64]);
    return wd_wave_min(t);
}

} // namespace

} // namespace str_er
