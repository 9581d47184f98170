// lattice_margin_kernels.h -- the launcher of the lattice decoder's margins (lattice_margin_kernels.hip; the rules are in
// lattice_margin_rules.h, the contract at str_er_lattice_margin in str_er.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/str_er.h"

namespace str_er {

constexpr int LM_WORDS = 4;        // words of a workgroup: a wave each
constexpr int LM_PARTS = 32;       // per-part entries of a word
constexpr int LM_FROM = 4;         // local nodes an edge into a node can leave
constexpr int LM_READINGS = 66;    // marginals of an edge

// What k_lattice_decode read (bigram [66 x 66] on the device, splits, the rows, first_run / n_of / slot [n_words]) and what it left for
// these words (dec [n_words x 8], chars and src [n_words x 64], parts at the words' slots) -> margins [n_words] (str_er_lattice_margin),
// read_margin and cut_margin [n_words x 32] int32, read, alt and cut_alt [n_words x 32] bytes, edge_min [n_words x 32 x 4] int32 and
// marginals [n_words x 32 x 4 x 66] int32 (null: not made).  The words must lie inside the runs: the caller checks.
void launch_lattice_margin(hipStream_t s, const uint8_t *bigram, int ins, int del, int split, const str_er_run_split *splits, const uint8_t *run_costs,
                           const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of, const int32_t *slot, int n_words, const int32_t *dec,
                           const uint8_t *chars, const uint8_t *src, const int32_t *parts, void *margins, int32_t *read_margin, int32_t *cut_margin, uint8_t *read,
                           uint8_t *alt, uint8_t *cut_alt, int32_t *edge_min, int32_t *marginals);

} // namespace str_er
