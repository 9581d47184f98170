// word_margin_kernels.h -- the launcher of the word decoder's margins (word_margin_kernels.hip; the rules are in word_margin_rules.h,
// the contract at str_er_word_margin in str_er.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace str_er {

constexpr int WG_WORDS = 4;        // words of a workgroup: a wave each

// bigram [66 x 66] (device), costs [n_runs x 65], first_run / n_of [n_words] and what k_word_decode left for these words (dec, chars
// and src [n_words x 64]) -> margins [n_words] (str_er_word_margin), row_margin [n_words x 32] int32, row_read and row_alt
// [n_words x 32] bytes, marginals [n_words x 32 x 66] int32 (null: not made).  The words must lie inside the cost rows: the caller checks.
void launch_word_margin(hipStream_t s, const uint8_t *bigram, int ins, int del, const uint8_t *costs, const int32_t *first_run, const int32_t *n_of, int n_words,
                        const void *dec, const uint8_t *chars, const uint8_t *src, void *margins, int32_t *row_margin, uint8_t *row_read, uint8_t *row_alt,
                        int32_t *marginals);

} // namespace str_er
