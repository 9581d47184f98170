// lattice_track_rules.h -- INTERNAL: the rules of the track match over the members' piece lattices (the contract is at
// str_er_lattice_track_member in str_er.h): the union of the members' lattice bands and one track against a lexicon with every member's
// backtrack for the winning entry.  HIP-free and header-only, composed from lattice_match_rules.h (the lattice, the cost of an entry, the
// table and its backtrack, the free cost) and track_read_rules.h (the tracks' checks, the member limit): the host entry point
// (api_lattice_track.cpp: str_er_lattice_match_tracks_host) and tests/cpp/lattice_track_rules_check.cpp use this same code;
// lattice_track_kernels.hip states the same rules for the device and is held against the numpy reference (tests/lattice_track_ref.py),
// which is written from the definition.
#pragma once
#include "lattice_match_rules.h"
#include "track_read_rules.h"

#include <vector>

namespace str_er_lt {

namespace lm = str_er_lm;
namespace tr = str_er_tr;
namespace wm = str_er_wm;

// bit l - 1 set iff an entry of length l (1 .. 32) is in the lattice band of a member of R runs and N nodes
inline uint32_t len_mask_of(int64_t R, int64_t N, int band)
{
    uint32_t mask = 0;
    for (int l = 1; l <= wm::MAX_LEN; ++l)
        if (lm::in_band(R, N, l, band)) mask |= 1u << (l - 1);
    return mask;
}

// One track against the whole lexicon on one thread: the members are `count` word indices.  member[i] receives the record of slot i
// with first_part left 0, src + 32 * i its source bytes, and the parts of slot i are appended to parts.
inline str_er_track_match match_track(const str_er_run_split *splits, const uint8_t *run_costs, const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of,
                                      const int32_t *members, int32_t count, const uint8_t *labels, const int32_t *offsets, int32_t n, const lm::Params &p, bool fold,
                                      str_er_lattice_track_member *member, uint8_t *src, std::vector<str_er_split_part> &parts)
{
    std::vector<lm::Lattice> lat((size_t)count);
    std::vector<char>        usable((size_t)count, 0);
    uint32_t                 mask = 0;
    uint32_t                 free_c = 0;
    int32_t                  n_used = 0;
    for (int32_t i = 0; i < count; ++i) {
        const int32_t w = members[i];
        const int64_t N = lm::word_nodes(splits, first_run[w], n_of[w]);
        free_c += (uint32_t)lm::free_cost(splits, run_costs, piece_costs, first_run[w], n_of[w], p.split);
        member[i] = str_er_lattice_track_member{-1, 0, 0, 0, 0, w};
        memset(src + (size_t)lm::SRC_BYTES * (size_t)i, 0xFF, lm::SRC_BYTES);
        if (N > lm::MAX_NODES) continue;
        usable[(size_t)i] = 1;
        ++n_used;
        mask |= len_mask_of(n_of[w], N, p.band);
        lm::build(lat[(size_t)i], splits, run_costs, piece_costs, first_run[w], n_of[w]);
    }
    wm::Best2 b;
    int32_t   tried = 0;
    for (int32_t e = 0; e < n; ++e) {
        const int len = offsets[e + 1] - offsets[e];
        if (!(mask >> (len - 1) & 1u)) continue;
        ++tried;
        int32_t sum = 0;
        for (int32_t i = 0; i < count; ++i)
            if (usable[(size_t)i]) sum += lm::entry_cost(lat[(size_t)i], labels + offsets[e], len, p, fold);
        b.add(wm::make_key(sum, e));
    }
    const str_er_word_match r = wm::make_match(b, (int32_t)free_c, tried);
    str_er_track_match      t{r.entry, r.cost, r.second_entry, r.second_cost, r.free_cost, r.n_tried, n_used, -1};
    int32_t                 best = -1;
    for (int32_t i = 0; i < count && t.entry >= 0; ++i) {
        if (!usable[(size_t)i]) continue;
        lm::Table         T;
        str_er_split_part own[lm::MAX_NODES];
        const uint8_t    *e = labels + offsets[t.entry];
        const int         len = offsets[t.entry + 1] - offsets[t.entry];
        str_er_lattice_track_member &M = member[i];
        M.cost = lm::fill_table(lat[(size_t)i], e, len, p, fold, T);
        M.n_parts = lm::backtrack(lat[(size_t)i], e, len, p, fold, T, own, src + (size_t)lm::SRC_BYTES * (size_t)i, &M.n_del, &M.n_ins);
        parts.insert(parts.end(), own, own + M.n_parts);
        if (best < 0 || M.cost < member[best].cost) best = i;
    }
    t.best_member = best < 0 ? -1 : members[best];
    return t;
}

} // namespace str_er_lt
