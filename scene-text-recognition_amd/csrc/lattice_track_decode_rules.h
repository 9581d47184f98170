// lattice_track_decode_rules.h -- INTERNAL: the rules of the track decode over the members' piece lattices (the contract is at
// str_er_lattice_track_decode in str_er.h): the prefix and suffix tables of the lattice recurrence for one member over its nodes, the
// cost of every single edit of a string from them and the member's edges, the seeds and the polish of one track on one thread with
// every member's backtrack for the final string.  HIP-free and header-only, composed from lattice_match_rules.h (the lattice, the
// table of a string and its backtrack), lattice_decode_rules.h (the seeds' strings) and track_decode_rules.h (lm, the neighbours and
// their numbering, the checks): the host entry point (api_lattice_track_decode.cpp: str_er_lattice_decode_tracks_host) and
// tests/cpp/lattice_track_decode_rules_check.cpp use this same code; lattice_track_decode_kernels.hip states the same rules for the
// device and is held against the numpy reference (tests/lattice_track_decode_ref.py), which is written from the definition and scores
// every neighbour with the full recurrence.
#pragma once
#include "lattice_decode_rules.h"
#include "lattice_match_rules.h"
#include "track_decode_rules.h"

#include <algorithm>
#include <vector>

namespace str_er_ltd {

namespace lm = str_er_lm;
namespace ld = str_er_ld;
namespace td = str_er_td;

constexpr int ALPHABET = td::ALPHABET, MAX_LEN = td::MAX_LEN, MAX_SEEDS = td::MAX_SEEDS, MAX_NODES = lm::MAX_NODES;
static_assert(MAX_LEN == lm::SRC_BYTES && MAX_NODES == ld::MAX_NODES, "a string's characters have a source byte each; the decoder's lattice is the matcher's");

inline bool params_ok(int32_t ins, int32_t del, int32_t rounds, int32_t split) { return td::params_ok(ins, del, rounds) && split >= 0 && split <= 255; }

// The tables of one member for the string s over its nodes: F.D[n][j] the cost of the first j labels with the path at node n (the
// table of str_er_lattice_match for s), G[g][n] the cost of the labels from g on from node n to N; F.D[N][l] = G[0][0] = L(s).
struct Tables {
    lm::Table F;
    int32_t   G[MAX_LEN + 1][MAX_NODES + 1];
};

inline void make_tables(const lm::Lattice &L, const uint8_t *s, int l, const lm::Params &p, Tables &T)
{
    lm::fill_table(L, s, l, p, false, T.F);
    for (int g = l; g >= 0; --g) T.G[g][L.N] = (l - g) * p.ins;
    for (int n = L.N - 1; n >= 0; --n)
        for (int g = l; g >= 0; --g) {
            int32_t best = INT32_MAX;
            for (int t = n + 1; t <= L.N && t <= n + lm::rs::MAX_ATOMS; ++t) {          // the edges that leave n: into the nodes t of the run n lies in or begins
                const int i = n - L.off[t];
                if (i < 0) break;
                const int32_t pen = i > 0 ? p.split : 0;
                if (g < l) best = std::min(best, T.G[g + 1][t] + (int32_t)L.row[t][i][s[g]] + pen);
                best = std::min(best, T.G[g][t] + p.del + pen);
            }
            if (g < l) best = std::min(best, T.G[g + 1][n] + p.ins);
            T.G[g][n] = best;
        }
}

// the cost of the string made of the first j labels, then the label a (a < 0: none), then the labels from g on: without a the two parts
// meet at any node; a is inserted at a node or read from an edge
inline int32_t joined_cost(const Tables &T, const lm::Lattice &L, int j, int a, int g, const lm::Params &p)
{
    int32_t best = INT32_MAX;
    for (int n = 0; n <= L.N; ++n) best = std::min(best, T.F.D[n][j] + T.G[g][n] + (a >= 0 ? p.ins : 0));
    if (a >= 0)
        for (int n = 1; n <= L.N; ++n)
            for (int i = 0; i < L.j[n]; ++i)
                best = std::min(best, T.F.D[L.off[n] + i][j] + (int32_t)L.row[n][i][a] + (i > 0 ? p.split : 0) + T.G[g][n]);
    return best;
}

// One track on one thread: the members are `count` word indices; dec[w] with its 64 label bytes at dchars + 64 * w is word w's
// str_er_lattice_decode.  p: this output's INS and DEL and SPLIT (the band is not read).  chars: 32 bytes; member[i] receives the record
// of slot i with first_part left 0, src + 32 * i its source bytes, and the parts of slot i are appended to parts.
inline str_er_track_decode decode_track(const str_er_run_split *splits, const uint8_t *run_costs, const uint8_t *piece_costs, const int32_t *first_run,
                                        const int32_t *n_of, const int32_t *members, int32_t count, const str_er_lattice_decode *dec, const uint8_t *dchars,
                                        const uint8_t *B, const lm::Params &p, int32_t rounds, uint8_t *chars, str_er_lattice_track_member *member, uint8_t *src,
                                        std::vector<str_er_split_part> &parts)
{
    str_er_track_decode r{-1, -1, 0, 0, 0, 0, -1, -1};
    memset(chars, 0xFF, MAX_LEN);
    std::vector<lm::Lattice> lat((size_t)count);
    std::vector<int32_t>     usable;          // slots
    int32_t                  seeds[MAX_SEEDS];
    int                      n_seeds = 0;
    for (int32_t i = 0; i < count; ++i) {
        const int32_t w = members[i];
        member[i] = str_er_lattice_track_member{-1, 0, 0, 0, 0, w};
        memset(src + (size_t)lm::SRC_BYTES * (size_t)i, 0xFF, lm::SRC_BYTES);
        if (lm::word_nodes(splits, first_run[w], n_of[w]) > MAX_NODES) continue;
        lm::build(lat[(size_t)i], splits, run_costs, piece_costs, first_run[w], n_of[w]);
        usable.push_back(i);
        if (n_seeds < MAX_SEEDS && dec[w].n_chars >= 1 && dec[w].n_chars <= MAX_LEN) seeds[n_seeds++] = i;
    }
    r.n_used = (int32_t)usable.size();
    if (n_seeds == 0) return r;
    const auto score = [&](const uint8_t *s, int l) {
        int32_t J = td::lm_cost(s, l, B);
        for (const int32_t i : usable) J += lm::entry_cost(lat[(size_t)i], s, l, p, false);
        return J;
    };
    uint8_t s[MAX_LEN + 1];
    int     l = 0;
    int32_t J = 0;
    for (int k = 0; k < n_seeds; ++k) {          // the smallest (J, seed rank)
        const int32_t  w = members[seeds[k]];
        const uint8_t *t = dchars + (size_t)w * ld::MAX_CHARS;
        const int32_t  Jk = score(t, dec[w].n_chars);
        if (k == 0 || Jk < J) { J = Jk; l = dec[w].n_chars; memcpy(s, t, (size_t)l); r.seed_member = w; }
    }
    r.seed_cost = J;
    std::vector<int32_t> acc(td::N_NEIGHBOURS);
    std::vector<Tables>  T(1);
    for (int round = 1; round <= rounds; ++round) {
        std::fill(acc.begin(), acc.end(), 0);
        for (const int32_t i : usable) {
            make_tables(lat[(size_t)i], s, l, p, T[0]);
            for (int x = 0; x < td::N_NEIGHBOURS; ++x) {
                int j, a, g;
                if (td::neighbour(x, l, j, a, g)) acc[(size_t)x] += joined_cost(T[0], lat[(size_t)i], j, a, g, p);
            }
        }
        int     best = -1;
        int32_t Jb = 0;
        uint8_t t[MAX_LEN + 1];
        for (int x = 0; x < td::N_NEIGHBOURS; ++x) {
            int j, a, g;
            if (!td::neighbour(x, l, j, a, g)) continue;
            const int     n = td::apply_neighbour(s, l, j, a, g, t);
            const int32_t Jx = td::lm_cost(t, n, B) + acc[(size_t)x];
            if (best < 0 || Jx < Jb) { best = x; Jb = Jx; }
        }
        if (best < 0 || Jb >= J) { r.converged = 1; break; }
        int j, a, g;
        td::neighbour(best, l, j, a, g);
        l = td::apply_neighbour(s, l, j, a, g, t);
        memcpy(s, t, (size_t)l);
        J = Jb;
        ++r.n_edits;
    }
    r.cost = J; r.n_chars = l; r.lm_cost = td::lm_cost(s, l, B);
    memcpy(chars, s, (size_t)l);
    for (const int32_t i : usable) {          // every member's own table and backtrack for the final string
        str_er_split_part            own[MAX_NODES];
        str_er_lattice_track_member &M = member[i];
        M.cost = lm::fill_table(lat[(size_t)i], s, l, p, false, T[0].F);
        M.n_parts = lm::backtrack(lat[(size_t)i], s, l, p, false, T[0].F, own, src + (size_t)lm::SRC_BYTES * (size_t)i, &M.n_del, &M.n_ins);
        parts.insert(parts.end(), own, own + M.n_parts);
    }
    return r;
}

} // namespace str_er_ltd
