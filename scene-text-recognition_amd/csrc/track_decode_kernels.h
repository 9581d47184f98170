// track_decode_kernels.h -- the launcher of the track decode (track_decode_kernels.hip; the rules are in track_decode_rules.h, the
// contract at str_er_track_decode in str_er.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace str_er {

// bigram [66 x 66] (device), costs [n_rows x 65], first_run / n_of [n_words], dec [n_words x 6 int32] (str_er_word_decode) and dchars
// [n_words x 64] as k_word_decode left them for these rows, track g = members[track_first[g] .. track_first[g] + track_count[g]) ->
// out [n_tracks x 8 int32] (str_er_track_decode), chars [n_tracks x 32] and member_cost for every slot of a track.  The words must lie
// inside the cost rows, the members inside the words and no track may have more than 1024 members: the caller checks.
void launch_track_decode(hipStream_t s, const uint8_t *bigram, int ins, int del, int rounds, const uint8_t *costs, const int32_t *first_run, const int32_t *n_of,
                         const void *dec, const uint8_t *dchars, const int32_t *track_first, const int32_t *track_count, const int32_t *members, int n_tracks,
                         void *out, uint8_t *chars, int32_t *member_cost);

} // namespace str_er
