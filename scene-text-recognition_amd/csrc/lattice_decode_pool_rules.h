// lattice_decode_pool_rules.h -- INTERNAL: the rules of the lattice decode pool (the contract is at "The lattice decode pool" in
// str_er.h): the geometry of a cell of the store, which piece of a call goes to which piece row of a cell and what a rebased split
// record is, and a pool on one thread (add, join, clear, read) built from ld::decode_word and ltd::decode_track.  HIP-free and
// header-only, on top of decode_pool_rules.h (keys, keep, the merge of kept lists) and lattice_track_decode_rules.h:
// tests/cpp/lattice_decode_pool_rules_check.cpp holds the one-thread pool against ltd::decode_track on explicitly concatenated and
// truncated member lists; lattice_decode_pool_kernels.hip states the same rules for the device and api_track_pool.cpp lays the store out
// from these strides.  The checks of an addition's slots, of a join and of the 65536-member limit are the track pool's
// (track_pool_rules.h).
#pragma once
#include "decode_pool_rules.h"
#include "lattice_track_decode_rules.h"

namespace str_er_ldp {

namespace dp = str_er_dp;
namespace ld = str_er_ld;
namespace lm = str_er_lm;
namespace ltd = str_er_ltd;
namespace rs = str_er_rs;

// A cell holds one kept member, the "word" of the track decode over lattices.  A usable member has N <= 32 nodes: at most 32 runs (a run
// has an atom at least), and at most 72 pieces (8 runs of 4 atoms with 9 pieces each; a run of A atoms has A (A + 1) / 2 - 1 pieces and
// A nodes, and 9 / 4 is the largest ratio).  The decode kernels address a row as base + 65 * index, so a cell's block of piece rows has
// to start at a multiple of 65 bytes, and the 16-byte stores of the copies want a multiple of 16: the block is 80 rows, 5200 = 65 * 80
// = 16 * 325 bytes, of which the first 72 can be used.  The run rows are the decode pool's 32 rows, 2080 bytes.
constexpr int CELL_RUNS = 32, CELL_PIECES_USED = 72, CELL_PIECES = 80, ALPHABET = 65;
constexpr int CELL_RUN_BYTES = CELL_RUNS * ALPHABET, CELL_PIECE_BYTES = CELL_PIECES * ALPHABET, CELL_SPLIT_BYTES = CELL_RUNS * (int)sizeof(str_er_run_split);
constexpr int TAB_BYTES = 4 * (3 + 33 + 128);          // a word's row of the structure table (LT_TAB_INTS int32)
// bytes of a kept member on the device: rows, split records, structure row, key, first run, run count, the decoder's record and labels
constexpr int CELL_BYTES = CELL_RUN_BYTES + CELL_PIECE_BYTES + CELL_SPLIT_BYTES + TAB_BYTES + 8 + 4 + 4 + (int)sizeof(str_er_lattice_decode) + ld::MAX_CHARS;
// cap_tracks * keep.  The structure table of the track decode keeps a piece's row as index | 2^30 (LM_PIECE in lattice_match_device.h)
// and masks the flag off again, so a piece row index has to stay below 2^30: 80 * cell + 79 < 2^30, at most 13 421 772 cells (the
// decode pool of rows allows 2^24; the run row index 32 * cell is far below either bound).
constexpr int64_t PIECE_FLAG = 1ll << 30;
constexpr int64_t MAX_CELLS = PIECE_FLAG / CELL_PIECES;
constexpr int64_t MAX_STORE_BYTES = 1ll << 40;
static_assert(CELL_RUN_BYTES % 16 == 0 && CELL_PIECE_BYTES % 16 == 0 && CELL_SPLIT_BYTES % 16 == 0 && TAB_BYTES % 16 == 0, "cells start on 16-byte boundaries");
static_assert(CELL_BYTES == 9072 && sizeof(str_er_run_split) == 32 && MAX_CELLS == 13421772 && CELL_PIECES * MAX_CELLS <= PIECE_FLAG && MAX_CELLS < dp::MAX_CELLS, "cell layout");
static_assert(8 * (rs::MAX_ATOMS * (rs::MAX_ATOMS + 1) / 2 - 1) == CELL_PIECES_USED && lm::MAX_NODES / rs::MAX_ATOMS == 8, "the pieces of a usable member");

inline bool create_ok(int64_t cap_tracks, int64_t keep) { return dp::create_ok(cap_tracks, keep); }
inline bool cells_fit(int64_t cap_tracks, int64_t keep) { return cap_tracks * keep <= MAX_CELLS && cap_tracks * keep * CELL_BYTES + 4 * cap_tracks <= MAX_STORE_BYTES; }

// a usable member: N <= 32, N = 0 included (the rule of str_er_lattice_track_decode)
inline bool usable(const str_er_run_split *splits, int32_t first_run, int32_t n_of) { return lm::word_nodes(splits, first_run, n_of) <= lm::MAX_NODES; }

// The rebasing rule.  The pieces of a member's runs go to the cell's piece rows back to back in run order, whatever their places in the
// call's piece table are: the pieces of the member's run t start at the cell's piece row piece_base(splits of the word, t), and piece k
// of that run (the call's row first_piece + k) is the row piece_base + k.
inline int32_t piece_base(const str_er_run_split *word_splits, int32_t t)
{
    int32_t b = 0;
    for (int32_t r = 0; r < t; ++r) b += word_splits[r].n_pieces;
    return b;
}
// ... and the split record of that run in a cell whose piece rows start at the row `cell_first_piece` of the table it is read with
// (80 * cell in the store, 80 * age rank in what a read's parts index, 0 in what _lattice_members hands back): every field but
// first_piece as it came
inline str_er_run_split rebased(const str_er_run_split &S, int32_t cell_first_piece, int32_t base)
{
    str_er_run_split R = S;
    R.first_piece = cell_first_piece + base;
    return R;
}

// what a slot keeps of a member; the split records are rebased to the member's own piece rows (cell_first_piece = 0)
struct Member {
    uint64_t              key = 0;
    int32_t               n_runs = 0;
    str_er_run_split      splits[CELL_RUNS] = {};
    uint8_t               run_rows[CELL_RUN_BYTES] = {};
    uint8_t               piece_rows[CELL_PIECE_BYTES] = {};
    str_er_lattice_decode dec{};
    uint8_t               chars[ld::MAX_CHARS] = {};
};

// the member made from the call's word (usable: the caller checks), its strings decoded on its own rows
inline Member make_member(uint64_t key, const str_er_run_split *splits, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t first_run, int32_t n_of,
                          const uint8_t *B, int32_t dec_ins, int32_t dec_del, int32_t split)
{
    Member x;
    x.key = key;
    x.n_runs = n_of;
    for (int32_t t = 0; t < n_of; ++t) {
        const str_er_run_split &S = splits[first_run + t];
        const int32_t           b = piece_base(splits + first_run, t);
        x.splits[t] = rebased(S, 0, b);
        memcpy(x.run_rows + (size_t)t * ALPHABET, run_costs + (size_t)(first_run + t) * ALPHABET, ALPHABET);
        if (S.n_pieces > 0) memcpy(x.piece_rows + (size_t)b * ALPHABET, piece_costs + (size_t)S.first_piece * ALPHABET, (size_t)S.n_pieces * ALPHABET);
    }
    uint8_t           src[ld::MAX_CHARS];
    str_er_split_part parts[ld::MAX_NODES + 1];
    x.dec = ld::decode_word(x.splits, x.run_rows, x.piece_rows, 0, n_of, B, dec_ins, dec_del, split, x.chars, src, parts);
    x.dec.first_part = 0;
    return x;
}

// what a read of a kept list gives
struct Read {
    str_er_pool_decode                       rec{};
    uint8_t                                  chars[ltd::MAX_LEN];
    std::vector<int32_t>                     member_cost;          // keep values, -1 past the kept members
    std::vector<str_er_lattice_track_member> members;              // per kept member in age order; word: the age rank
    std::vector<uint8_t>                     src;                  // 32 bytes a kept member
    std::vector<str_er_split_part>           parts;                // run 32 * rank + t, piece 80 * rank + the member's piece row
};

// the record of a kept list: ltd::decode_track on the members numbered 0 .. n - 1 in the list's order, member i at the runs 32 * i and
// the piece rows 80 * i
inline Read read_list(const std::vector<Member> &kept, int32_t n_members, int keep, const uint8_t *B, int32_t ins, int32_t del, int32_t rounds, int32_t split)
{
    const size_t                       n = kept.size();
    std::vector<str_er_run_split>      splits(n * CELL_RUNS + 1);
    std::vector<uint8_t>               run_rows(n * CELL_RUN_BYTES + 1), piece_rows(n * CELL_PIECE_BYTES + 1), dchars(n * ld::MAX_CHARS + 1);
    std::vector<int32_t>               first(n + 1), n_of(n + 1), members(n + 1);
    std::vector<str_er_lattice_decode> dec(n + 1);
    for (size_t i = 0; i < n; ++i) {
        for (int t = 0; t < CELL_RUNS; ++t) splits[i * CELL_RUNS + t] = rebased(kept[i].splits[t], (int32_t)(i * CELL_PIECES), kept[i].splits[t].first_piece);
        memcpy(run_rows.data() + i * CELL_RUN_BYTES, kept[i].run_rows, CELL_RUN_BYTES);
        memcpy(piece_rows.data() + i * CELL_PIECE_BYTES, kept[i].piece_rows, CELL_PIECE_BYTES);
        memcpy(dchars.data() + i * ld::MAX_CHARS, kept[i].chars, ld::MAX_CHARS);
        first[i] = (int32_t)(i * CELL_RUNS); n_of[i] = kept[i].n_runs; members[i] = (int32_t)i; dec[i] = kept[i].dec;
    }
    Read R;
    R.members.assign(n + 1, str_er_lattice_track_member{-1, 0, 0, 0, 0, -1});
    R.src.assign((n + 1) * lm::SRC_BYTES, 0xFF);
    const lm::Params          p{ins, del, 0, split};
    const str_er_track_decode r = ltd::decode_track(splits.data(), run_rows.data(), piece_rows.data(), first.data(), n_of.data(), members.data(), (int32_t)n, dec.data(),
                                                    dchars.data(), B, p, rounds, R.chars, R.members.data(), R.src.data(), R.parts);
    R.members.resize(n);
    R.src.resize(n * lm::SRC_BYTES);
    R.member_cost.assign((size_t)keep, -1);
    int32_t fp = 0;
    for (size_t i = 0; i < n; ++i) {
        R.member_cost[i] = R.members[i].cost;
        R.members[i].first_part = fp;
        fp += R.members[i].n_parts;
    }
    R.rec = str_er_pool_decode{r.cost, r.seed_cost, r.n_chars, r.n_edits, r.converged, r.n_used, r.seed_member, r.lm_cost, n_members, (int32_t)n};
    return R;
}

// A lattice decode pool on one thread.  The table B (66 x 66) stays the caller's.
struct KeepPool {
    int            keep = 1;
    const uint8_t *B = nullptr;
    int32_t        dec_ins = 0, dec_del = 0, ins = 64, del = 64, rounds = 8, split = 8;
    uint32_t       serial = 0;
    std::vector<std::vector<Member>> kept;          // per slot, ascending keys
    std::vector<int32_t>             n_members;

    KeepPool(int32_t cap, int keep_, const uint8_t *B_, int32_t dec_ins_, int32_t dec_del_, int32_t ins_, int32_t del_, int32_t rounds_, int32_t split_)
        : keep(keep_), B(B_), dec_ins(dec_ins_), dec_del(dec_del_), ins(ins_), del(del_), rounds(rounds_), split(split_), kept((size_t)cap), n_members((size_t)cap, 0) {}

    // one addition: track g of the call goes to slots[g]
    void add(const str_er_run_split *splits, const uint8_t *run_costs, const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of,
             const int32_t *track_first, const int32_t *track_count, const int32_t *members, int32_t n_tracks, const int32_t *slots)
    {
        if (n_tracks <= 0) return;
        ++serial;
        for (int32_t g = 0; g < n_tracks; ++g) {
            std::vector<Member> in;
            for (int32_t j = 0; j < track_count[g]; ++j) {
                const int32_t w = members[track_first[g] + j];
                if (!usable(splits, first_run[w], n_of[w])) continue;
                in.push_back(make_member(dp::make_key(serial, track_first[g] + j), splits, run_costs, piece_costs, first_run[w], n_of[w], B, dec_ins, dec_del, split));
            }
            dp::merge_keep(kept[(size_t)slots[g]], in, keep);
            n_members[(size_t)slots[g]] += track_count[g];
        }
    }

    void clear(int32_t slot)
    {
        kept[(size_t)slot].clear();
        n_members[(size_t)slot] = 0;
    }

    void join(int32_t dst, const int32_t *srcs, int32_t n_srcs)
    {
        for (int32_t k = 0; k < n_srcs; ++k) {
            dp::merge_keep(kept[(size_t)dst], kept[(size_t)srcs[k]], keep);
            n_members[(size_t)dst] += n_members[(size_t)srcs[k]];
            clear(srcs[k]);
        }
    }

    void reset()
    {
        for (size_t s = 0; s < kept.size(); ++s) clear((int32_t)s);
        serial = 0;
    }

    Read read(int32_t slot) const { return read_list(kept[(size_t)slot], n_members[(size_t)slot], keep, B, ins, del, rounds, split); }
};

} // namespace str_er_ldp
