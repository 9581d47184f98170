// word_decode_kernels.h -- the launcher of the open-vocabulary word decoder (word_decode_kernels.hip; the rules are in
// word_decode_rules.h, the contract at str_er_word_decode in str_er.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace str_er {

constexpr int WD_WORDS = 4;        // words of a workgroup: a wave each

// bigram [66 x 66] (device), costs [n_runs x 65], first_run / n_of [n_words] -> dec [n_words] (str_er_word_decode), chars and src
// [n_words x 64].  The words must lie inside the cost rows: the caller checks.
void launch_word_decode(hipStream_t s, const uint8_t *bigram, int ins, int del, const uint8_t *costs, const int32_t *first_run, const int32_t *n_of, int n_words,
                        void *dec, uint8_t *chars, uint8_t *src);

} // namespace str_er
