// lattice_decode_kernels.h -- the launcher of the joint decode over the piece lattice (lattice_decode_kernels.hip; the rules are in
// lattice_decode_rules.h, the contract at str_er_lattice_decode in str_er.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/str_er.h"

namespace str_er {

constexpr int LD_WORDS = 4;        // words of a workgroup: a wave each

// bigram [66 x 66] (device); splits [n_runs], run_costs [n_runs x 65], piece_costs [n_pieces x 65], first_run / n_of / slot [n_words]:
// what k_split_words reads -> dec [n_words x 8 int32] (str_er_lattice_decode, first_part left 0), chars and src [n_words x 64], parts
// [n_slots x 2 int32] from the word's slot on.  The words must lie inside the runs, the pieces inside the rows and slot[w] must be the
// atoms of the words before w: the caller checks.
void launch_lattice_decode(hipStream_t s, const uint8_t *bigram, int ins, int del, int split, const str_er_run_split *splits, const uint8_t *run_costs,
                           const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of, const int32_t *slot, int n_words, int32_t *dec, uint8_t *chars,
                           uint8_t *src, int32_t *parts);

} // namespace str_er
