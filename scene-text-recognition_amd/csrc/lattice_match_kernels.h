// lattice_match_kernels.h -- the launcher of the lexicon match over the piece lattice (lattice_match_kernels.hip; the rules are in
// lattice_match_rules.h, the contract at str_er_lattice_match in str_er.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/str_er.h"
#include "word_match_kernels.h"

namespace str_er {

constexpr int LM_FINAL_WORDS = 4;        // words of a workgroup of k_lattice_match_final: a wave each

// lex, p: the matcher's (wm_chunks(lex) chunks a word); splits [n_runs], run_costs [n_runs x 65], piece_costs [n_pieces x 65], first_run /
// n_of / slot [n_words]: what k_split_words reads, the rows as they are (the fold is applied when they are staged) -> partial
// [n_words x wm_chunks x 2] keys -> matches [n_words x 10 int32] (str_er_lattice_match, first_part left 0), src [n_words x 32], parts
// [n_slots x 2 int32] from the word's slot on.  The words must lie inside the runs, the pieces inside the rows and slot[w] must be the
// atoms of the words before w: the caller checks.
void launch_lattice_match(hipStream_t s, const WmLexDev &lex, const WmParams &p, int split, const str_er_run_split *splits, const uint8_t *run_costs,
                          const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of, const int32_t *slot, int n_words, uint64_t *partial,
                          int32_t *matches, uint8_t *src, int32_t *parts);

} // namespace str_er
