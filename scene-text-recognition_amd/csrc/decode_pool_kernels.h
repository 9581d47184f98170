// decode_pool_kernels.h -- the launchers of the decode pool (decode_pool_kernels.hip; the rules are in decode_pool_rules.h, the
// contract at str_er_pool_decode in str_er.h).  The reading itself is launch_track_decode (track_decode_kernels.h) on the pool's store.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace str_er {

constexpr int DP_CELL_ROW_BYTES = 32 * 65;      // the rows of a cell: 2080 bytes, a multiple of 16

// The pool on the device.  Slot s has the cells s * keep .. s * keep + keep - 1; cell w is the "word" w of launch_track_decode: its
// rows at costs + w * 2080 (first_run[w] = 32 * w, written once), its run count n_of[w], the decoder's record dec + 6 * w and the 64
// label bytes dchars + 64 * w; key[w] is 0 where the cell is empty.  n_members [cap]: everything ever added to the slot.
struct DpPoolDev {
    uint8_t  *costs;
    uint64_t *key;
    int32_t  *first_run, *n_of, *dec;
    uint8_t  *dchars;
    int32_t  *n_members;
    int32_t   cap, keep;
};

// every cell empty, every count 0, first_run written
void launch_dpool_reset(hipStream_t s, const DpPoolDev &pool);
// Track g of the call (members[track_first[g] .. + track_count[g]) of the words of costs / first_run / n_of, with the decoder's records
// dec [n_words x 6] and labels dchars [n_words x 64] made on these rows) goes to the slot slots[g] under the keys serial << 32 | index
// in the member array: the slots are distinct and inside the pool, the caller checks.
void launch_dpool_keep(hipStream_t s, const DpPoolDev &pool, uint32_t serial, const uint8_t *costs, const int32_t *first_run, const int32_t *n_of, const void *dec,
                       const uint8_t *dchars, const int32_t *track_first, const int32_t *track_count, const int32_t *members, const int32_t *slots, int n_tracks);
// dst keeps the newest of its own and the srcs' [n_srcs] kept members (distinct slots, dst not among them); the srcs become empty
void launch_dpool_join(hipStream_t s, const DpPoolDev &pool, int dst, const int32_t *srcs, int n_srcs);
// the slots [n] (any, also repeated) become empty
void launch_dpool_clear(hipStream_t s, const DpPoolDev &pool, const int32_t *slots, int n);
// The plan of a read of the slots [n] (any, also repeated): request i is the track i with track_first[i] = i * keep, track_count[i] =
// its kept members and members[i * keep ..] the cells in ascending key order; rank_of [n x keep]: the age rank of the cell c of
// request i at i * keep + c; member_cost [n x keep] preset to -1.
void launch_dpool_plan(hipStream_t s, const DpPoolDev &pool, const int32_t *slots, int n, int32_t *track_first, int32_t *track_count, int32_t *members, int32_t *rank_of,
                       int32_t *member_cost);
// behind launch_track_decode: rec [n x 8 int32] (str_er_track_decode, seed_member a cell) -> out [n x 10 int32] (str_er_pool_decode,
// seed_member an age rank)
void launch_dpool_records(hipStream_t s, const DpPoolDev &pool, const int32_t *slots, int n, const int32_t *rec, const int32_t *track_count, const int32_t *rank_of,
                          int32_t *out);

} // namespace str_er
