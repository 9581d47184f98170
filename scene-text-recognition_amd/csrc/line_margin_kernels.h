// line_margin_kernels.h -- the launcher of the line decoder's margins (line_margin_kernels.hip; the rules are in line_margin_rules.h,
// the contract at str_er_line_margin in str_er.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "line_decode_kernels.h"

namespace str_er {

constexpr int LM_FW_ROW = 136;        // uint32 of a row of the forward table: V_{i-1} in 0 .. 65, X_i at 66, S_i from 68 on
constexpr int LM_MARGINALS = 68;      // int32 of a row of the marginals: the 65 readings, dropped, join, break

// Behind launch_line_decode on the same stream, with its arguments and what it left (dec, chars, src) -> margins [n_lines]
// (str_er_line_margin), row_margin and gap_margin [n_rows] int32, row_read, row_alt and gap_move [n_rows] bytes, marginals (null: not
// made) [n_rows x 68] int32; fw [n_rows x LM_FW_ROW] uint32 is scratch.  LD_LINES lines a workgroup, a wave each.  Every line writes
// the slices of its own rows alone; what lies in no line is left as it is.
void launch_line_margin(hipStream_t s, const uint8_t *bigram, int ins, int del, const uint8_t *costs, const uint8_t *gaps, const int32_t *first_row, const int32_t *n_of,
                        const int32_t *row_map, int n_lines, const void *dec, const uint8_t *chars, const uint16_t *src, uint32_t *fw, void *margins, int32_t *row_margin,
                        uint8_t *row_read, uint8_t *row_alt, int32_t *gap_margin, uint8_t *gap_move, int32_t *marginals);

} // namespace str_er
