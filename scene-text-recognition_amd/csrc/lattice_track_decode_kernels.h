// lattice_track_decode_kernels.h -- the launcher of the track decode over the members' piece lattices (lattice_track_decode_kernels.hip;
// the rules are in lattice_track_decode_rules.h, the contract at str_er_lattice_track_decode in str_er.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/str_er.h"
#include "lattice_track_kernels.h"

namespace str_er {

// bigram [66 x 66] (device); ins, del, rounds: the track decode's; split: SPLIT; splits, run_costs, piece_costs, first_run / n_of
// [n_words]: what k_lattice_decode reads; dec [n_words x 8 int32] (str_er_lattice_decode) and dchars [n_words x 64] as k_lattice_decode
// left them for these rows.  Track g has the members members[track_first[g] .. track_first[g] + track_count[g]); slot_track
// [n_members]: the track of every slot of the member array, -1 for a slot of no track; pslot [n_members]: the part slot of every slot,
// the sum of the N <= 32 of the slots before it -> tab [n_words x LT_TAB_INTS] (the structure of every word, made once by
// k_lattice_track_table), out [n_tracks x 8 int32] (str_er_track_decode), chars [n_tracks x 32], mrec [n_members x 6 int32]
// (str_er_lattice_track_member, first_part left 0), src [n_members x 32], parts [part slots x 2 int32] from the slot's part slot on.  The
// words must lie inside the runs, the pieces inside the rows, the members inside the words, the tracks inside the member array and no
// track may have more than 1024 members: the caller checks.
void launch_lattice_track_decode(hipStream_t s, const uint8_t *bigram, int ins, int del, int rounds, int split, const str_er_run_split *splits, const uint8_t *run_costs,
                                 const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of, int n_words, const void *dec, const uint8_t *dchars,
                                 const int32_t *track_first, const int32_t *track_count, const int32_t *members, const int32_t *slot_track, const int32_t *pslot,
                                 int n_members, int n_tracks, int32_t *tab, void *out, uint8_t *chars, int32_t *mrec, uint8_t *src, int32_t *parts);
// The two steps on their own: launch_lattice_track_table (lattice_track_kernels.h) makes tab, and this one decodes on a tab that is
// given -- the rows of the words the members name must have been made with the same del and split.  The lattice decode pool keeps a
// row per cell of its store and makes those of the cells it reads.
void launch_lattice_track_decode_tab(hipStream_t s, const uint8_t *bigram, int ins, int del, int rounds, int split, const str_er_run_split *splits, const uint8_t *run_costs,
                                     const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of, const void *dec, const uint8_t *dchars,
                                     const int32_t *track_first, const int32_t *track_count, const int32_t *members, const int32_t *slot_track, const int32_t *pslot,
                                     int n_members, int n_tracks, const int32_t *tab, void *out, uint8_t *chars, int32_t *mrec, uint8_t *src, int32_t *parts);

} // namespace str_er
