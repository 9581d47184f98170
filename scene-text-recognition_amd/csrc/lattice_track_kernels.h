// lattice_track_kernels.h -- the launcher of the track match over the members' piece lattices (lattice_track_kernels.hip; the rules are in
// lattice_track_rules.h, the contract at str_er_lattice_track_member in str_er.h).  The lexicon on the device is the matcher's
// (word_match_kernels.h), the chunks are the track match's (track_match_kernels.h: tm_chunks).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/str_er.h"
#include "track_match_kernels.h"

namespace str_er {

constexpr int LT_TAB_INTS = 3 + 33 + 128;        // int32 of a word's structure in the table: N, S0, S1, d0[33], erow[128]

// k_lattice_track_table alone: tab [n_words x LT_TAB_INTS], the structure of every word (the track pool stages its members through it)
void launch_lattice_track_table(hipStream_t s, int del, int split, const str_er_run_split *splits, const int32_t *first_run, const int32_t *n_of, int n_words, int32_t *tab);
// lex, p, split: the matcher's and SPLIT; splits, run_costs, piece_costs, first_run / n_of [n_words]: what k_lattice_match reads.  Track g
// has the members members[track_first[g] .. track_first[g] + track_count[g]); slot_track [n_members]: the track of every slot of the
// member array, -1 for a slot of no track; pslot [n_members]: the part slot of every slot, the sum of the N <= 32 of the slots before it
// -> tab [n_words x LT_TAB_INTS] (the structure of every word, made once), partial [n_tracks x tm_chunks x 2] keys -> matches [n_tracks x 8
// int32] (str_er_track_match), mrec [n_members x 6 int32] (str_er_lattice_track_member, first_part left 0), src [n_members x 32], parts
// [part slots x 2 int32] from the slot's part slot on; mfree [n_members]: the slots' free costs, between the kernels.  The words must
// lie inside the runs, the pieces inside the rows, the members inside the words and the tracks inside the member array: the caller checks.
void launch_lattice_track(hipStream_t s, const WmLexDev &lex, const WmParams &p, int split, const str_er_run_split *splits, const uint8_t *run_costs,
                          const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of, int n_words, const int32_t *track_first, const int32_t *track_count,
                          const int32_t *members, const int32_t *slot_track, const int32_t *pslot, int n_members, int n_tracks, int32_t *tab, uint64_t *partial,
                          int32_t *matches, int32_t *mrec, uint8_t *src, int32_t *parts, int32_t *mfree);

} // namespace str_er
