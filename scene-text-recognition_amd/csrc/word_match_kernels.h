// word_match_kernels.h -- the device lexicon and the launchers of the lexicon matcher (word_match_kernels.hip; the rules are in
// word_match_rules.h, the contract at str_er_word_match in str_er.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace str_er {

constexpr int WM_GROUP = 64;              // entries of one length that a wave takes at a time: one lane each
constexpr int WM_CHUNK_GROUPS = 64;       // groups of a (word, chunk) workgroup
constexpr int WM_CHUNK = WM_GROUP * WM_CHUNK_GROUPS;      // the chunk size in entries (str_er_lexicon_info)

// The lexicon on the device: sorted by length, stable by index, every length padded to whole groups.  Group g of length len holds
// ceil(len / 4) rows of 64 words at chars + goff[g]: word q of lane l = the labels 4q .. 4q + 3 of the lane's entry, lowest byte
// first, so that a wave's load of four characters of its 64 entries is one contiguous 256 bytes.
struct WmLexDev {
    const uint32_t *chars;
    const uint32_t *goff;       // [n_groups] first word of a group
    const int32_t  *index;      // [n_groups x 64] the entry's index as the caller gave it, -1 in the padding
    const int32_t  *len_first;  // [34] [len] first group of length len (1 .. 32), [33] = n_groups, [0] = 0
    const int32_t  *len_count;  // [34] [len] entries shorter than len, [33] = n
    int32_t n_groups;
    int32_t fold;               // the lexicon's fold-case flag
    const int32_t  *pos;        // [n] the slot g * 64 + lane of entry i in `index`: its inverse (the track match reads the winner's labels by it)
};

struct WmParams { int32_t ins, del, band; };

// prob [n x k] (f64) -> cost [n x 65]: the cost rows of n runs with the model's labels (device, k of them)
void launch_run_costs(hipStream_t s, const double *prob, int n, int k, const int32_t *labels, bool fold, uint8_t *cost);
// chunks of a word: as many as the widest band of lengths can need
int wm_chunks(const WmLexDev &lex);
// costs [n_runs x 65], first_run / n_of [n_words] -> partial [n_words x wm_chunks x 2] keys -> matches [n_words] (str_er_word_match)
void launch_word_match(hipStream_t s, const WmLexDev &lex, const WmParams &p, const uint8_t *costs, const int32_t *first_run, const int32_t *n_of, int n_words,
                       uint64_t *partial, void *matches);

} // namespace str_er
