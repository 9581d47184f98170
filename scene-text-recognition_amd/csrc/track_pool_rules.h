// track_pool_rules.h -- INTERNAL: the rules of the track pool (the contract is at str_er_pool_match in str_er.h): the state of a slot
// and its merge, the checks of the slots of an addition and of a join with the member limit, and a pool on one thread over explicit
// accumulator rows (add, join, clear, read), built from wm::entry_cost and the lattice rule.  HIP-free and header-only, on top of
// track_read_rules.h and lattice_track_rules.h: api_track_pool.cpp runs the checks from here, tests/cpp/track_pool_rules_check.cpp holds
// the one-thread pool against tr::match_track and lt::match_track on the concatenated member lists; track_pool_kernels.hip states the
// same sums for the device.
#pragma once
#include "lattice_track_rules.h"

#include <vector>

namespace str_er_tp {

namespace lm = str_er_lm;
namespace lt = str_er_lt;
namespace tr = str_er_tr;
namespace wm = str_er_wm;

// what a slot holds beside its accumulator row
struct SlotState {
    uint32_t mask = 0;          // bit l - 1: the entries of length l are tried
    int32_t  free_cost = 0, n_used = 0, n_members = 0;
};

inline void merge(SlotState &a, const SlotState &b)
{
    a.mask |= b.mask; a.free_cost += b.free_cost; a.n_used += b.n_used; a.n_members += b.n_members;
}

// a slot of `have` members takes `add` more (both >= 0)
inline bool members_fit(int64_t have, int64_t add) { return have + add <= tr::MAX_MEMBERS; }

// The slots of an addition against the members every slot has (n_members_of: cap values): STR_ER_EINVAL on a slot out of range or named
// twice, STR_ER_ECAPACITY where a slot would pass the limit.  seen: scratch of cap bytes, all zero before and after.
inline int add_check(const int32_t *slots, const int32_t *track_count, int32_t n_tracks, const int32_t *n_members_of, int32_t cap, std::vector<uint8_t> &seen)
{
    int rc = STR_ER_OK, done = 0;
    for (; done < n_tracks && rc == STR_ER_OK; ++done) {
        const int32_t s = slots[done];
        if (s < 0 || s >= cap || seen[(size_t)s]) { rc = STR_ER_EINVAL; break; }
        seen[(size_t)s] = 1;
    }
    for (int32_t g = 0; g < done; ++g) seen[(size_t)slots[g]] = 0;
    for (int32_t g = 0; g < n_tracks && rc == STR_ER_OK; ++g)
        if (!members_fit(n_members_of[slots[g]], track_count[g])) rc = STR_ER_ECAPACITY;
    return rc;
}

// a join of srcs into dst: STR_ER_EINVAL on a slot out of range, a repeated slot or dst among the srcs, STR_ER_ECAPACITY above the limit
inline int join_check(int32_t dst, const int32_t *srcs, int32_t n_srcs, const int32_t *n_members_of, int32_t cap, std::vector<uint8_t> &seen)
{
    if (dst < 0 || dst >= cap) return STR_ER_EINVAL;
    int     rc = STR_ER_OK, done = 0;
    int64_t total = n_members_of[dst];
    seen[(size_t)dst] = 1;
    for (; done < n_srcs; ++done) {
        const int32_t s = srcs[done];
        if (s < 0 || s >= cap || seen[(size_t)s]) { rc = STR_ER_EINVAL; break; }
        seen[(size_t)s] = 1;
        total += n_members_of[s];
    }
    seen[(size_t)dst] = 0;
    for (int32_t k = 0; k < done; ++k) seen[(size_t)srcs[k]] = 0;
    if (rc == STR_ER_OK && total > tr::MAX_MEMBERS) rc = STR_ER_ECAPACITY;
    return rc;
}

// the record of a slot from its accumulator row (one int32 per entry of the lexicon, in the caller's order) and its state
inline str_er_pool_match read_slot(const int32_t *acc, const SlotState &st, const int32_t *offsets, int32_t n)
{
    wm::Best2 b;
    int32_t   tried = 0;
    for (int32_t e = 0; e < n; ++e) {
        const int len = offsets[e + 1] - offsets[e];
        if (!(st.mask >> (len - 1) & 1u)) continue;
        ++tried;
        b.add(wm::make_key(acc[e], e));
    }
    const str_er_word_match r = wm::make_match(b, st.free_cost, tried);
    return str_er_pool_match{r.entry, r.cost, r.second_entry, r.second_cost, r.free_cost, r.n_tried, st.n_used, st.n_members};
}

// A pool on one thread.  The lexicon (entries as labels, offsets[n + 1]) and the cost rows stay the caller's.
struct Pool {
    const uint8_t *labels = nullptr;
    const int32_t *offsets = nullptr;
    int32_t        n = 0;
    lm::Params     p;
    bool           fold = false;
    std::vector<std::vector<int32_t>> acc;
    std::vector<SlotState>            st;

    Pool(int32_t cap, const uint8_t *labels_, const int32_t *offsets_, int32_t n_, const lm::Params &p_, bool fold_)
        : labels(labels_), offsets(offsets_), n(n_), p(p_), fold(fold_), acc((size_t)cap, std::vector<int32_t>((size_t)n_, 0)), st((size_t)cap) {}

    // `count` members (word indices) on their cost rows: every usable member's distance to every entry, whatever its length
    void add(int32_t slot, const uint8_t *costs, const int32_t *first_run, const int32_t *n_of, const int32_t *members, int32_t count)
    {
        SlotState s;
        for (int32_t i = 0; i < count; ++i) {
            const int32_t  w = members[i], m = n_of[w];
            const uint8_t *C = costs + (size_t)first_run[w] * wm::ALPHABET;
            s.mask |= tr::len_mask_of(m, p.band);
            s.free_cost += wm::free_cost(C, m);
            ++s.n_members;
            if (m > wm::MAX_LEN) continue;
            ++s.n_used;
            for (int32_t e = 0; e < n; ++e) acc[(size_t)slot][(size_t)e] += wm::entry_cost(C, m, labels + offsets[e], offsets[e + 1] - offsets[e], p.ins, p.del, fold);
        }
        merge(st[(size_t)slot], s);
    }

    // ... over their piece lattices
    void add_lattice(int32_t slot, const str_er_run_split *splits, const uint8_t *run_costs, const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of,
                     const int32_t *members, int32_t count)
    {
        SlotState s;
        for (int32_t i = 0; i < count; ++i) {
            const int32_t w = members[i];
            const int64_t N = lm::word_nodes(splits, first_run[w], n_of[w]);
            s.free_cost += lm::free_cost(splits, run_costs, piece_costs, first_run[w], n_of[w], p.split);
            ++s.n_members;
            if (N > lm::MAX_NODES) continue;
            ++s.n_used;
            s.mask |= lt::len_mask_of(n_of[w], N, p.band);
            lm::Lattice L;
            lm::build(L, splits, run_costs, piece_costs, first_run[w], n_of[w]);
            for (int32_t e = 0; e < n; ++e) acc[(size_t)slot][(size_t)e] += lm::entry_cost(L, labels + offsets[e], offsets[e + 1] - offsets[e], p, fold);
        }
        merge(st[(size_t)slot], s);
    }

    void clear(int32_t slot)
    {
        std::fill(acc[(size_t)slot].begin(), acc[(size_t)slot].end(), 0);
        st[(size_t)slot] = SlotState{};
    }

    void join(int32_t dst, const int32_t *srcs, int32_t n_srcs)
    {
        for (int32_t k = 0; k < n_srcs; ++k) {
            for (int32_t e = 0; e < n; ++e) acc[(size_t)dst][(size_t)e] += acc[(size_t)srcs[k]][(size_t)e];
            merge(st[(size_t)dst], st[(size_t)srcs[k]]);
            clear(srcs[k]);
        }
    }

    str_er_pool_match read(int32_t slot) const { return read_slot(acc[(size_t)slot].data(), st[(size_t)slot], offsets, n); }
};

} // namespace str_er_tp
