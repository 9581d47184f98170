// decode_pool_rules.h -- INTERNAL: the rules of the decode pool (the contract is at str_er_pool_decode in str_er.h): the key of a
// member, the kept list of a slot and its merge (the `keep` largest keys of a union), and a pool on one thread (add, join, clear, read)
// built from wd::decode_word and td::decode_track.  HIP-free and header-only, on top of track_decode_rules.h:
// tests/cpp/decode_pool_rules_check.cpp holds the one-thread pool against td::decode_track on explicitly concatenated and truncated
// member lists; decode_pool_kernels.hip states the same rules for the device.  The checks of an addition's slots, of a join and of the
// 65536-member limit are the track pool's (track_pool_rules.h) and run in api_track_pool.cpp on the host's mirror of the member counts.
#pragma once
#include "track_decode_rules.h"

#include <algorithm>
#include <iterator>
#include <vector>

namespace str_er_dp {

namespace td = str_er_td;
namespace wd = str_er_wd;

constexpr int MAX_KEEP = td::MAX_MEMBERS;                    // kept members of a slot: what one track decode takes
constexpr int CELL_ROWS = td::MAX_LEN;                       // rows of a cell: a usable member has at most 32
constexpr int CELL_ROW_BYTES = CELL_ROWS * td::ALPHABET;     // 2080, a multiple of 16
constexpr int64_t MAX_CELLS = 1ll << 24;                     // cap_tracks * keep: the row index 32 * cell stays an int32
static_assert(CELL_ROW_BYTES == 2080 && CELL_ROW_BYTES % 16 == 0, "cell layout");

inline bool create_ok(int64_t cap_tracks, int64_t keep) { return cap_tracks >= 1 && keep >= 1 && keep <= MAX_KEEP; }
inline bool cells_fit(int64_t cap_tracks, int64_t keep) { return cap_tracks * keep <= MAX_CELLS; }

// the key of the member at `index` of the member array of the pool's serial-th addition (serial >= 1): never 0, unique in a pool, and
// larger is newer
inline uint64_t make_key(uint32_t serial, int32_t index) { return (uint64_t)serial << 32 | (uint32_t)index; }

// a usable member (at most 32 rows): whether the call's word w is one
inline bool usable(int32_t n_runs) { return n_runs <= td::MAX_LEN; }

// what a slot keeps of a member
struct Member {
    uint64_t           key = 0;
    int32_t            n_runs = 0;
    uint8_t            rows[CELL_ROW_BYTES] = {};
    str_er_word_decode dec{};
    uint8_t            chars[wd::MAX_CHARS] = {};
};

// The kept list a (ascending keys) takes the list b (ascending keys, none of them in a): the `keep` largest of the union, ascending.
// The `keep` largest of a union are the `keep` largest of the union of the lists' own `keep` largest, so the result does not depend on
// how a sequence of merges is grouped.
template <typename M> inline void merge_keep(std::vector<M> &a, const std::vector<M> &b, int keep)
{
    std::vector<M> u;
    u.reserve(a.size() + b.size());
    std::merge(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(u), [](const M &x, const M &y) { return x.key < y.key; });
    if ((int64_t)u.size() > keep) u.erase(u.begin(), u.end() - keep);
    a.swap(u);
}

// the record of a kept list: td::decode_track on the members numbered 0 .. n - 1 in the list's order; chars: 32 bytes, member_cost:
// n values
inline str_er_pool_decode read_list(const std::vector<Member> &kept, int32_t n_members, const uint8_t *B, int32_t ins, int32_t del, int32_t rounds, uint8_t *chars,
                                    int32_t *member_cost)
{
    const size_t                    n = kept.size();
    std::vector<uint8_t>            costs(n * CELL_ROW_BYTES + 1), dchars(n * wd::MAX_CHARS + 1);
    std::vector<int32_t>            first(n + 1), n_of(n + 1), members(n + 1);
    std::vector<str_er_word_decode> dec(n + 1);
    for (size_t i = 0; i < n; ++i) {
        memcpy(costs.data() + i * CELL_ROW_BYTES, kept[i].rows, CELL_ROW_BYTES);
        memcpy(dchars.data() + i * wd::MAX_CHARS, kept[i].chars, wd::MAX_CHARS);
        first[i] = (int32_t)(i * CELL_ROWS); n_of[i] = kept[i].n_runs; members[i] = (int32_t)i; dec[i] = kept[i].dec;
    }
    const str_er_track_decode r = td::decode_track(costs.data(), first.data(), n_of.data(), members.data(), (int32_t)n, dec.data(), dchars.data(), B, ins, del, rounds, chars,
                                                   member_cost);
    return str_er_pool_decode{r.cost, r.seed_cost, r.n_chars, r.n_edits, r.converged, r.n_used, r.seed_member, r.lm_cost, n_members, (int32_t)n};
}

// A decode pool on one thread.  The table B (66 x 66) stays the caller's.
struct KeepPool {
    int            keep = 1;
    const uint8_t *B = nullptr;
    int32_t        dec_ins = 0, dec_del = 0, ins = 64, del = 64, rounds = 8;
    uint32_t       serial = 0;
    std::vector<std::vector<Member>> kept;          // per slot, ascending keys
    std::vector<int32_t>             n_members;

    KeepPool(int32_t cap, int keep_, const uint8_t *B_, int32_t dec_ins_, int32_t dec_del_, int32_t ins_, int32_t del_, int32_t rounds_)
        : keep(keep_), B(B_), dec_ins(dec_ins_), dec_del(dec_del_), ins(ins_), del(del_), rounds(rounds_), kept((size_t)cap), n_members((size_t)cap, 0) {}

    // one addition: track g of the call (members[track_first[g] .. + track_count[g]), words of costs / first_run / n_of) goes to slots[g]
    void add(const uint8_t *costs, const int32_t *first_run, const int32_t *n_of, const int32_t *track_first, const int32_t *track_count, const int32_t *members,
             int32_t n_tracks, const int32_t *slots)
    {
        if (n_tracks <= 0) return;
        ++serial;
        uint8_t src[wd::MAX_CHARS];
        for (int32_t g = 0; g < n_tracks; ++g) {
            std::vector<Member> in;
            for (int32_t j = 0; j < track_count[g]; ++j) {
                const int32_t w = members[track_first[g] + j], m = n_of[w];
                if (!usable(m)) continue;
                Member x;
                x.key = make_key(serial, track_first[g] + j);
                x.n_runs = m;
                if (m > 0) memcpy(x.rows, costs + (size_t)first_run[w] * td::ALPHABET, (size_t)m * td::ALPHABET);
                x.dec = wd::decode_word(x.rows, m, B, dec_ins, dec_del, x.chars, src);
                in.push_back(x);
            }
            merge_keep(kept[(size_t)slots[g]], in, keep);
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
            merge_keep(kept[(size_t)dst], kept[(size_t)srcs[k]], keep);
            n_members[(size_t)dst] += n_members[(size_t)srcs[k]];
            clear(srcs[k]);
        }
    }

    void reset()
    {
        for (size_t s = 0; s < kept.size(); ++s) clear((int32_t)s);
        serial = 0;
    }

    // chars: 32 bytes; member_cost: keep values, -1 past the kept members
    str_er_pool_decode read(int32_t slot, uint8_t *chars, int32_t *member_cost) const
    {
        std::fill(member_cost, member_cost + keep, -1);
        return read_list(kept[(size_t)slot], n_members[(size_t)slot], B, ins, del, rounds, chars, member_cost);
    }
};

} // namespace str_er_dp
