// line_decode_kernels.h -- the launcher of the line decoder (line_decode_kernels.hip; the rules are in line_decode_rules.h, the contract
// at str_er_line_decode in str_er.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace str_er {

constexpr int LD_LINES = 4;        // lines of a workgroup: a wave each
constexpr int LD_BP_ROW = 68;      // uint16 of a row of the back-pointer table: the run step's 66 states, the gap's word, one unused

// bigram [66 x 66] (device), costs [n_rows x 65], gaps [n_rows x 2], first_row / n_of [n_lines] -> dec [n_lines] (str_er_line_decode),
// chars and src [3 x n_rows], word_of_row [n_rows]; bp [n_rows x LD_BP_ROW] is scratch.  row_map (null: row r is cost row r) [n_rows]:
// the cost row of every row, for rows that do not lie back to back in costs (the parts' rows of a detect call); it must stay inside
// costs.  Every line writes the slices of its own rows alone: the lines must lie inside the rows and not overlap, the caller checks.
// What lies in no line is left as it is.
void launch_line_decode(hipStream_t s, const uint8_t *bigram, int ins, int del, const uint8_t *costs, const uint8_t *gaps, const int32_t *first_row, const int32_t *n_of,
                        const int32_t *row_map, int n_lines, uint16_t *bp, void *dec, uint8_t *chars, uint16_t *src, int32_t *word_of_row);

} // namespace str_er
