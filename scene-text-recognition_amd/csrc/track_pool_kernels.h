// track_pool_kernels.h -- the launchers of the track pool (track_pool_kernels.hip; the rules are in track_pool_rules.h, the contract at
// str_er_pool_match in str_er.h).  The lexicon on the device is the matcher's (word_match_kernels.h), the chunks are the track match's
// (track_match_kernels.h: tm_chunks).
#pragma once
#include "lattice_track_kernels.h"

namespace str_er {

constexpr int TP_STATE_INTS = 4;      // int32 of a slot's state: the mask of lengths tried, the free cost, the usable members, the members

// The pool on the device: slot s has the accumulator row acc + s * row_ints (row_ints = lex.n_groups * 64: one int32 per slot of the
// padded lexicon, as lex.index lays them out) and the state state + s * TP_STATE_INTS.
struct TpPoolDev {
    int32_t *acc, *state;
    int32_t  row_ints;
};

// Track g of the call (members[track_first[g] .. track_first[g] + track_count[g]) of the words of costs / first_run / n_of, as for
// launch_track_match) is added to the slot slots[g]: the slots are distinct and inside the pool, the caller checks.
void launch_pool_add(hipStream_t s, const WmLexDev &lex, const WmParams &p, const TpPoolDev &pool, const uint8_t *costs, const int32_t *first_run, const int32_t *n_of,
                     const int32_t *track_first, const int32_t *track_count, const int32_t *members, const int32_t *slots, int n_tracks);
// ... over the members' piece lattices, what launch_lattice_track reads; tab [n_words x LT_TAB_INTS] is made here
void launch_pool_add_lattice(hipStream_t s, const WmLexDev &lex, const WmParams &p, int split, const TpPoolDev &pool, const str_er_run_split *splits,
                             const uint8_t *run_costs, const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of, int n_words, const int32_t *track_first,
                             const int32_t *track_count, const int32_t *members, const int32_t *slots, int n_tracks, int32_t *tab);
// slots [n] (any, also repeated) -> partial [n x tm_chunks x 2] keys -> out [n x 8 int32] (str_er_pool_match)
void launch_pool_read(hipStream_t s, const WmLexDev &lex, const TpPoolDev &pool, const int32_t *slots, int n, uint64_t *partial, int32_t *out);
// dst += the slots srcs [n_srcs] (distinct, dst not among them), which become empty
void launch_pool_join(hipStream_t s, const TpPoolDev &pool, int dst, const int32_t *srcs, int n_srcs);
// the slots [n] (any, also repeated) become empty
void launch_pool_clear(hipStream_t s, const TpPoolDev &pool, const int32_t *slots, int n);

} // namespace str_er
