// track_decode_rules.h -- INTERNAL: the rules of the track decode (the contract is at str_er_track_decode in str_er.h): the checks of its
// arguments, the bigram cost of a string, the prefix and suffix tables of the matcher's recurrence for one member, the cost of every
// single edit of a string from them, the seeds and the polish of one track on one thread.  HIP-free and header-only, on top of
// word_decode_rules.h (the seeds' strings) and word_match_rules.h (the recurrence): the host entry point (api_track_decode.cpp:
// str_er_decode_tracks_host), the argument checks of the device entry point and tests/cpp/track_decode_rules_check.cpp use this same
// code; track_decode_kernels.hip states the same rules for the device and is held against the numpy reference
// (tests/track_decode_ref.py), which is written from the definition and scores every neighbour with the full recurrence.
#pragma once
#include "word_decode_rules.h"

#include <string.h>

#include <vector>

namespace str_er_td {

namespace wm = str_er_wm;
namespace wd = str_er_wd;

constexpr int ALPHABET = wm::ALPHABET, E = wd::E, STATES = wd::STATES;
constexpr int MAX_LEN = 32;               // labels of a string, rows of a usable member
constexpr int MAX_SEEDS = 32;
constexpr int MAX_MEMBERS = 1024;         // of one track: the loop over them runs inside one workgroup
constexpr int MAX_ROUNDS = 64;
// the neighbours of a string: SUB(j, a) at j * 65 + a, DEL(j) at DEL_AT + j, INS(j, a) at INS_AT + j * 65 + a
constexpr int DEL_AT = MAX_LEN * ALPHABET, INS_AT = DEL_AT + MAX_LEN, N_NEIGHBOURS = INS_AT + (MAX_LEN + 1) * ALPHABET;
static_assert(DEL_AT == 2080 && INS_AT == 2112 && N_NEIGHBOURS == 4257, "neighbour numbering");

inline bool params_ok(int32_t ins, int32_t del, int32_t rounds) { return ins >= 1 && ins <= 255 && del >= 1 && del <= 255 && rounds >= 0 && rounds <= MAX_ROUNDS; }

// STR_ER_OK, or why not: the tracks ascend in the member array without overlap, none has more than 1024 members, the members are words
inline int tracks_check(const int32_t *track_first, const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks, int32_t n_words)
{
    int64_t at = 0;
    for (int32_t g = 0; g < n_tracks; ++g) {
        if (track_count[g] < 0 || track_first[g] < at || (int64_t)track_first[g] + track_count[g] > n_members) return STR_ER_EINVAL;
        if (track_count[g] > MAX_MEMBERS) return STR_ER_ECAPACITY;
        at = (int64_t)track_first[g] + track_count[g];
    }
    for (int32_t i = 0; i < n_members; ++i)
        if (members[i] < 0 || members[i] >= n_words) return STR_ER_EINVAL;
    return STR_ER_OK;
}

// lm(s) of the l >= 1 labels s under the table B
inline int32_t lm_cost(const uint8_t *s, int l, const uint8_t *B)
{
    int32_t c = B[E * STATES + s[0]] + B[s[l - 1] * STATES + E];
    for (int j = 0; j + 1 < l; ++j) c += B[s[j] * STATES + s[j + 1]];
    return c;
}

// A(s) = D[m][l] of the matcher's recurrence on the m <= 32 rows C, no band, no fold
inline int32_t align_cost(const uint8_t *C, int m, const uint8_t *s, int l, int32_t ins, int32_t del) { return wm::entry_cost(C, m, s, l, ins, del, false); }

// The tables of one member for the string s: F[j][i] the cost of the first j labels against the first i rows, G[j][i] the cost of
// the labels from j on against the rows from i on; F[l][m] = G[0][0] = A(s).
struct Tables {
    int32_t F[MAX_LEN + 1][MAX_LEN + 1], G[MAX_LEN + 1][MAX_LEN + 1];
};

inline void make_tables(const uint8_t *C, int m, const uint8_t *s, int l, int32_t ins, int32_t del, Tables &T)
{
    for (int i = 0; i <= m; ++i) { T.F[0][i] = i * del; T.G[l][i] = (m - i) * del; }
    for (int j = 1; j <= l; ++j) {
        T.F[j][0] = j * ins;
        for (int i = 1; i <= m; ++i) {
            const int32_t sub = T.F[j - 1][i - 1] + C[(size_t)(i - 1) * ALPHABET + s[j - 1]], up = T.F[j][i - 1] + del, left = T.F[j - 1][i] + ins;
            T.F[j][i] = sub < up ? (sub < left ? sub : left) : (up < left ? up : left);
        }
    }
    for (int j = l - 1; j >= 0; --j) {
        T.G[j][m] = (l - j) * ins;
        for (int i = m - 1; i >= 0; --i) {
            const int32_t sub = T.G[j + 1][i + 1] + C[(size_t)i * ALPHABET + s[j]], up = T.G[j][i + 1] + del, left = T.G[j + 1][i] + ins;
            T.G[j][i] = sub < up ? (sub < left ? sub : left) : (up < left ? up : left);
        }
    }
}

// the cost of the string made of the first j labels, then the label a (a < 0: none), then the labels from g on, from the tables: the
// label a takes a row of its own or is inserted; without it the two parts meet at any row
inline int32_t joined_cost(const Tables &T, const uint8_t *C, int m, int j, int a, int g, int32_t ins)
{
    int32_t best = INT32_MAX;
    for (int i = 0; i <= m; ++i) {
        int32_t v;
        if (a < 0) v = T.F[j][i] + T.G[g][i];
        else {
            v = T.F[j][i] + ins + T.G[g][i];
            if (i < m) {
                const int32_t w = T.F[j][i] + C[(size_t)i * ALPHABET + a] + T.G[g][i + 1];
                v = w < v ? w : v;
            }
        }
        best = v < best ? v : best;
    }
    return best;
}

// whether the neighbour `index` of a string of length l exists, and what it is: the labels before j stay, then a (-1: none), then the
// labels from g on
inline bool neighbour(int index, int l, int &j, int &a, int &g)
{
    if (index < DEL_AT) { j = index / ALPHABET; a = index % ALPHABET; g = j + 1; return j < l; }
    if (index < INS_AT) { j = index - DEL_AT; a = -1; g = j + 1; return l > 1 && j < l; }
    j = (index - INS_AT) / ALPHABET; a = (index - INS_AT) % ALPHABET; g = j;
    return l < MAX_LEN && j <= l;
}

inline int apply_neighbour(const uint8_t *s, int l, int j, int a, int g, uint8_t *out)
{
    int n = 0;
    for (int k = 0; k < j; ++k) out[n++] = s[k];
    if (a >= 0) out[n++] = (uint8_t)a;
    for (int k = g; k < l; ++k) out[n++] = s[k];
    return n;
}

// One track on one thread: the members are `count` word indices, word w has the rows first_run[w] .. first_run[w] + n_of[w] of costs
// and the decoder's record dec[w] with its 64 label bytes at dchars + 64 * w.  chars: 32 bytes; member_cost: count values.
inline str_er_track_decode decode_track(const uint8_t *costs, const int32_t *first_run, const int32_t *n_of, const int32_t *members, int32_t count,
                                        const str_er_word_decode *dec, const uint8_t *dchars, const uint8_t *B, int32_t ins, int32_t del, int32_t rounds,
                                        uint8_t *chars, int32_t *member_cost)
{
    str_er_track_decode r{-1, -1, 0, 0, 0, 0, -1, -1};
    memset(chars, 0xFF, MAX_LEN);
    std::vector<int32_t> usable;          // slots
    int32_t              seeds[MAX_SEEDS];
    int                  n_seeds = 0;
    for (int32_t i = 0; i < count; ++i) {
        member_cost[i] = -1;
        const int32_t w = members[i];
        if (n_of[w] > MAX_LEN) continue;
        usable.push_back(i);
        if (n_seeds < MAX_SEEDS && dec[w].n_chars >= 1 && dec[w].n_chars <= MAX_LEN) seeds[n_seeds++] = i;
    }
    r.n_used = (int32_t)usable.size();
    if (n_seeds == 0) return r;
    const auto rows = [&](int32_t slot) { return costs + (size_t)first_run[members[slot]] * ALPHABET; };
    const auto m_of = [&](int32_t slot) { return (int)n_of[members[slot]]; };
    const auto score = [&](const uint8_t *s, int l) {
        int32_t J = lm_cost(s, l, B);
        for (const int32_t i : usable) J += align_cost(rows(i), m_of(i), s, l, ins, del);
        return J;
    };
    uint8_t s[MAX_LEN + 1];
    int     l = 0;
    int32_t J = 0;
    for (int k = 0; k < n_seeds; ++k) {          // the set median: the smallest (J, seed rank)
        const int32_t  w = members[seeds[k]];
        const uint8_t *t = dchars + (size_t)w * wd::MAX_CHARS;
        const int32_t  Jk = score(t, dec[w].n_chars);
        if (k == 0 || Jk < J) { J = Jk; l = dec[w].n_chars; memcpy(s, t, (size_t)l); r.seed_member = w; }
    }
    r.seed_cost = J;
    std::vector<int32_t> acc(N_NEIGHBOURS);
    Tables               T;
    for (int round = 1; round <= rounds; ++round) {
        std::fill(acc.begin(), acc.end(), 0);
        for (const int32_t i : usable) {
            make_tables(rows(i), m_of(i), s, l, ins, del, T);
            for (int x = 0; x < N_NEIGHBOURS; ++x) {
                int j, a, g;
                if (neighbour(x, l, j, a, g)) acc[(size_t)x] += joined_cost(T, rows(i), m_of(i), j, a, g, ins);
            }
        }
        int     best = -1;
        int32_t Jb = 0;
        uint8_t t[MAX_LEN + 1];
        for (int x = 0; x < N_NEIGHBOURS; ++x) {
            int j, a, g;
            if (!neighbour(x, l, j, a, g)) continue;
            const int     n = apply_neighbour(s, l, j, a, g, t);
            const int32_t Jx = lm_cost(t, n, B) + acc[(size_t)x];
            if (best < 0 || Jx < Jb) { best = x; Jb = Jx; }
        }
        if (best < 0 || Jb >= J) { r.converged = 1; break; }
        int j, a, g;
        neighbour(best, l, j, a, g);
        l = apply_neighbour(s, l, j, a, g, t);
        memcpy(s, t, (size_t)l);
        J = Jb;
        ++r.n_edits;
    }
    r.cost = J; r.n_chars = l; r.lm_cost = lm_cost(s, l, B);
    memcpy(chars, s, (size_t)l);
    for (const int32_t i : usable) member_cost[i] = align_cost(rows(i), m_of(i), s, l, ins, del);
    return r;
}

} // namespace str_er_td
