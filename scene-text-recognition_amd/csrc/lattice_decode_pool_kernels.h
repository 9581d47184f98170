// lattice_decode_pool_kernels.h -- the launchers of the lattice decode pool (lattice_decode_pool_kernels.hip; the rules are in
// lattice_decode_pool_rules.h, the contract at "The lattice decode pool" in str_er.h).  The reading itself is
// launch_lattice_track_decode_tab (lattice_track_decode_kernels.h) on the pool's store, behind launch_dpool_plan (decode_pool_kernels.h)
// on the store's keys.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/str_er.h"
#include "decode_pool_kernels.h"

namespace str_er {

constexpr int LDP_CELL_RUNS = 32, LDP_CELL_PIECES = 80;                                                  // rows of a cell's two blocks
constexpr int LDP_MAX_CELLS = (1 << 30) / LDP_CELL_PIECES;                                              // 13 421 772: a piece row index 80 * cell + k stays below LM_PIECE
constexpr int LDP_CELL_RUN_BYTES = LDP_CELL_RUNS * 65, LDP_CELL_PIECE_BYTES = LDP_CELL_PIECES * 65;      // 2080 and 5200 bytes, multiples of 16 and of 65

// The pool on the device.  Slot s has the cells s * keep .. s * keep + keep - 1; cell w is the "word" w of launch_lattice_track_decode:
// its runs are the rows 32 * w .. of run_rows (first_run[w] = 32 * w, written once) with the split records splits + 32 * w, whose
// first_piece is 80 * w + the piece's row in the cell's block of piece_rows; n_of[w] its run count, dec + 8 * w the lattice decoder's
// record and dchars + 64 * w its 64 label bytes; tab + LT_TAB_INTS * w the word's row of the structure table, made by
// launch_ldpool_tracks for the cells of a read; key[w] is 0 where the cell is empty.  n_members [cap]: everything ever added to the slot.
struct LdpPoolDev {
    uint8_t          *run_rows, *piece_rows;
    str_er_run_split *splits;
    int32_t          *tab;
    uint64_t         *key;
    int32_t          *first_run, *n_of, *dec;
    uint8_t          *dchars;
    int32_t          *n_members;
    int32_t           cap, keep;
};

// the store's keys and counts as the decode pool's kernels that read nothing else take them (launch_dpool_plan, launch_dpool_clear)
inline DpPoolDev ldpool_keys(const LdpPoolDev &p)
{
    DpPoolDev d{};
    d.key = p.key; d.n_members = p.n_members; d.cap = p.cap; d.keep = p.keep;
    return d;
}

// every cell empty, every count 0, first_run written
void launch_ldpool_reset(hipStream_t s, const LdpPoolDev &pool);
// Track g of the call (members[track_first[g] .. + track_count[g]) of the words of splits / run_costs / piece_costs / first_run / n_of,
// with the lattice decoder's records dec [n_words x 8] and labels dchars [n_words x 64] made on these rows) goes to the slot slots[g]
// under the keys serial << 32 | index in the member array.  The slots are distinct and inside the pool, the split records are those
// rs::splits_ok passes (a run's pieces inside the piece rows): the caller checks.
void launch_ldpool_keep(hipStream_t s, const LdpPoolDev &pool, uint32_t serial, const str_er_run_split *splits, const uint8_t *run_costs, const uint8_t *piece_costs,
                        const int32_t *first_run, const int32_t *n_of, const void *dec, const uint8_t *dchars, const int32_t *track_first, const int32_t *track_count,
                        const int32_t *members, const int32_t *slots, int n_tracks);
// dst keeps the newest of its own and the srcs' [n_srcs] kept members (distinct slots, dst not among them); the srcs become empty
void launch_ldpool_join(hipStream_t s, const LdpPoolDev &pool, int dst, const int32_t *srcs, int n_srcs);
// Behind launch_dpool_plan for n requests: the member array of the read has n x keep slots, slot i * keep + r the r-th oldest kept cell
// of request i.  slot_track [n x keep]: i where r < track_count[i], else -1; pslot [n x keep]: 32 part slots each; and the structure
// row of every cell named, with the track decode's DEL and SPLIT, into the store: a read writes pool.tab and nothing else of the pool.
// lead [n]: 1 for the first request that names its slot, 0 for a repetition, which writes no row (one writer a row).
void launch_ldpool_tracks(hipStream_t s, const LdpPoolDev &pool, int del, int split, int n, const int32_t *lead, const int32_t *track_count, const int32_t *members, int32_t *slot_track,
                          int32_t *pslot);
// Behind launch_lattice_track_decode_tab: rec [n x 8 int32] (str_er_track_decode, seed_member a cell) -> out [n x 10 int32]
// (str_er_pool_decode, seed_member an age rank); the member records' word and the parts' runs and pieces from cells to age ranks (run
// 32 * rank + t, piece 80 * rank + row); member_cost [n x keep] (preset to -1) the kept members' costs.
void launch_ldpool_records(hipStream_t s, const LdpPoolDev &pool, const int32_t *slots, int n, const int32_t *rec, const int32_t *track_count, const int32_t *members,
                           const int32_t *rank_of, const int32_t *pslot, int32_t *out, int32_t *mrec, int32_t *parts, int32_t *member_cost);

} // namespace str_er
