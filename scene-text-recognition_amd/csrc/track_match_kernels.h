// track_match_kernels.h -- the launchers of the track match (track_match_kernels.hip; the rules are in track_read_rules.h, the contract
// at str_er_word_link in str_er.h).  The lexicon on the device is the matcher's (word_match_kernels.h).
#pragma once
#include "word_match_kernels.h"

namespace str_er {

// groups of a (track, chunk) workgroup: a quarter of the matcher's chunk.  A workgroup stays for all members of its track, and there
// are far fewer tracks than words: with the matcher's 64 groups the 125 tracks of profiles/track_read.md gave 1.2 rounds of
// workgroups on the device and the second round ran nearly empty.  (lattice_track_kernels.hip cuts the lexicon in the same way)
constexpr int TM_CHUNK_GROUPS = 16;
// chunks of a track: they cover the whole lexicon, since the lengths a track tries are a union of bands
int tm_chunks(const WmLexDev &lex);
// costs [rows x 65], first_run / n_of [words] as for launch_word_match; track g has the members members[track_first[g] ..
// track_first[g] + track_count[g]) -> partial [n_tracks x tm_chunks x 2] keys -> matches [n_tracks] (str_er_track_match) and
// member_cost, one per slot of the member array
void launch_track_match(hipStream_t s, const WmLexDev &lex, const WmParams &p, const uint8_t *costs, const int32_t *first_run, const int32_t *n_of,
                        const int32_t *track_first, const int32_t *track_count, const int32_t *members, int n_tracks, uint64_t *partial, void *matches,
                        int32_t *member_cost);

} // namespace str_er
