// line_lattice_kernels.h -- the launcher of the joint decode of a line over its runs' piece lattices (line_lattice_kernels.hip; the rules
// are in line_lattice_rules.h, the contract at str_er_line_lattice_decode in str_er.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/str_er.h"

namespace str_er {

constexpr int LL_LINES = 4;        // lines of a workgroup: a wave each
constexpr int LL_BP_ROW = 68;      // uint32 of a row of the back-pointer table: the node step's 66 states, the gap's word, the node's (j, A, run)

// bigram [66 x 66] (device), splits [n_runs], run_costs [n_runs x 65], piece_costs [n_pieces x 65], gaps [n_runs x 2], first_run / n_of /
// slot [n_lines] (slot: the atoms of all runs before the line's first) -> dec [n_lines] (str_er_line_lattice_decode, first_part 0),
// chars and src [3 x atoms], parts [atoms x 2] and word_of_part [atoms] at the lines' slots; bp [atoms x LL_BP_ROW] is scratch.  Every
// line writes the slices of its own nodes alone: the lines must lie inside the runs and not overlap, the records must hold 0 .. 3
// cuts and pieces inside piece_costs, the caller checks.  What lies in no line is left as it is.
void launch_line_lattice_decode(hipStream_t s, const uint8_t *bigram, int ins, int del, int split, const str_er_run_split *splits, const uint8_t *run_costs,
                                const uint8_t *piece_costs, const uint8_t *gaps, const int32_t *first_run, const int32_t *n_of, const int32_t *slot, int n_lines,
                                uint32_t *bp, int32_t *dec, uint8_t *chars, uint16_t *src, int32_t *parts, int32_t *word_of_part);

} // namespace str_er
