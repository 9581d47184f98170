// line_decode_rules_check.cpp -- the rules of the line decoder (csrc/line_decode_rules.h, the code the host entry points run) on the CPU,
// under the host sanitizers: the recurrence against an enumeration of every path on tables whose live part is 2 or 3 characters, the cost
// of the returned string recomputed from its labels and sources, the identities of the contract against the word decoder's rules
// (csrc/word_decode_rules.h), the row limit and its bound, the gap costs at their corners and the argument checks.  A program of its
// own; prints "<checks> checks, <wrong> wrong".
#include "../../scene-text-recognition_amd/csrc/line_decode_rules.h"

#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

namespace wd = str_er_wd;
namespace ld = str_er_ld;

static long n_checks = 0, n_wrong = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++n_checks;                                                                  \
        if (!(cond)) { ++n_wrong; std::printf("line %d: %s\n", __LINE__, #cond); }   \
    } while (0)

static int B_at(const uint8_t *B, int a, int b) { return B[a * wd::STATES + b]; }

// the cheapest path over the live characters 0 .. n - 1 by brute force: in front of every row but the first a join or a break (where it
// is on), per row a drop or a reading, and behind either one inserted character that follows some character (prev: the last character
// of the word so far, E for none)
static int32_t brute(const uint8_t *C, const uint8_t *G, int m, int i, int prev, const uint8_t *B, int n, int ins, int del)
{
    if (i == m) return B_at(B, prev, wd::E);
    int32_t best = 1 << 30;
    const auto row = [&](int32_t gap, int p0) {
        const auto tail = [&](int32_t sofar, int p) {
            best = std::min(best, sofar + brute(C, G, m, i + 1, p, B, n, ins, del));
            if (ins > 0 && p != wd::E)
                for (int c = 0; c < n; ++c) best = std::min(best, sofar + B_at(B, p, c) + ins + brute(C, G, m, i + 1, c, B, n, ins, del));
        };
        if (del > 0) tail(gap + del, p0);
        for (int b = 0; b < n; ++b) tail(gap + B_at(B, p0, b) + C[i * 65 + b], b);
    };
    if (i == 0) row(0, prev);
    else {
        if (G[2 * i] != ld::OFF) row(G[2 * i], prev);
        if (G[2 * i + 1] != ld::OFF) row(B_at(B, prev, wd::E) + G[2 * i + 1], wd::E);
    }
    return best;
}

// the cost of a returned string under the definition
static int32_t path_cost(const uint8_t *C, const uint8_t *G, int m, const uint8_t *B, const uint8_t *chars, const uint16_t *src, int n_chars, int ins, int del)
{
    int               prev = wd::E, used = 0;
    int32_t           s = 0;
    std::vector<char> broken((size_t)std::max(m, 1), 0);
    for (int k = 0; k < n_chars; ++k) {
        s += B_at(B, prev, chars[k]);
        const int r = src[k] & 0x3FFF;
        if (src[k] & ld::SRC_BREAK) { s += G[2 * r + 1]; broken[(size_t)r] = 1; }
        else if (src[k] & ld::SRC_INS) s += ins;
        else { s += C[r * 65 + chars[k]]; ++used; }
        prev = chars[k];
    }
    for (int i = 1; i < m; ++i)
        if (!broken[(size_t)i]) s += G[2 * i];
    return s + B_at(B, prev, wd::E) + del * (m - used);
}

int main()
{
    std::mt19937 rng(4321);
    const int    pairs[6][2] = {{0, 0}, {5, 0}, {0, 7}, {3, 4}, {1, 1}, {255, 255}};

    // small alphabets inside the full one: the other characters cost 255 everywhere and the live costs stay below 40, so that no path
    // through a dead character can win
    for (int n = 2; n <= 3; ++n)
        for (int m = 0; m <= 4; ++m)
            for (const auto &pr : pairs)
                for (int rep = 0; rep < (m == 4 ? 4 : 12); ++rep) {
                    const int             hi = rep % 2 ? 4 : 40;
                    const size_t          mm = (size_t)std::max(m, 1);
                    std::vector<uint8_t>  C(mm * 65, 255), B(wd::TABLE, 255), G(mm * 2), chars(3 * mm);
                    std::vector<uint16_t> src(3 * mm);
                    std::vector<int32_t>  wor(mm);
                    for (int i = 0; i < m; ++i) {
                        for (int a = 0; a < n; ++a) C[i * 65 + a] = (uint8_t)(rng() % hi);
                        G[2 * i] = (uint8_t)(rng() % hi); G[2 * i + 1] = (uint8_t)(rng() % hi);
                        if (rng() % 5 == 0) G[2 * i + rng() % 2] = 255;
                    }
                    for (int a = 0; a <= n; ++a)
                        for (int b = 0; b <= n; ++b) B[(a == n ? wd::E : a) * wd::STATES + (b == n ? wd::E : b)] = (uint8_t)(rng() % hi);
                    const int ins = pr[0], del = pr[1];
                    const str_er_line_decode r = ld::decode_line(C.data(), G.data(), m, B.data(), ins, del, chars.data(), src.data(), wor.data());
                    CHECK(r.cost == brute(C.data(), G.data(), m, 0, wd::E, B.data(), n, ins, del));
                    CHECK(r.cost == path_cost(C.data(), G.data(), m, B.data(), chars.data(), src.data(), r.n_chars, ins, del));
                    CHECK(r.n_sub + r.n_ins + r.n_breaks == r.n_chars && r.n_sub + r.n_del == m && r.n_chars <= std::max(0, 3 * m - 1));
                    CHECK((ins > 0 || r.n_ins == 0) && (del > 0 || r.n_del == 0));
                    for (int k = 0; k < 3 * m; ++k) CHECK(k < r.n_chars ? (chars[k] < n || chars[k] == wd::E) : (chars[k] == 0xFF && src[k] == 0xFFFF));
                    int at = 0;
                    for (int i = 0; i < m; ++i) {
                        CHECK(wor[i] == -1 || (wor[i] >= at && wor[i] <= r.n_breaks));
                        if (wor[i] >= 0) at = wor[i];
                    }
                }

    // the identities on the full alphabet: joins alone are the word decoder; a forced segmentation is its words, joined by one 65; free
    // gaps are never worse than it
    for (int it = 0; it < 120; ++it) {
        const auto &pr = pairs[it % 6];
        int        lengths[5], n_words = 1 + (int)(rng() % 5), m = 0;
        for (int w = 0; w < n_words; ++w) { lengths[w] = 1 + (int)(rng() % 8); m += lengths[w]; }
        std::vector<uint8_t>  C((size_t)m * 65), B(wd::TABLE), G((size_t)m * 2), F((size_t)m * 2), chars(3 * (size_t)m), want;
        std::vector<uint16_t> src(3 * (size_t)m);
        std::vector<int32_t>  wor((size_t)m);
        for (auto &v : C) v = (uint8_t)(rng() % 10 == 0 ? rng() % 24 : 60 + rng() % 196);
        for (auto &v : B) v = (uint8_t)(rng() % (it % 3 ? 256 : 6));
        for (auto &v : F) v = (uint8_t)(rng() % 255);
        int32_t total = 0, paid = 0;
        for (int w = 0, at = 0; w < n_words; at += lengths[w], ++w) {
            uint8_t wc[64], ws[64];
            const str_er_word_decode d = wd::decode_word(C.data() + (size_t)at * 65, lengths[w], B.data(), pr[0], pr[1], wc, ws);
            total += d.cost;
            if (w) want.push_back(65);
            want.insert(want.end(), wc, wc + d.n_chars);
            for (int k = 0; k < lengths[w]; ++k) {
                G[2 * (at + k)] = k ? 0 : 255; G[2 * (at + k) + 1] = k ? 255 : 0;
                if (at + k > 0) paid += F[2 * (at + k) + (k ? 0 : 1)];
            }
            if (n_words == 1) {          // (1): record, labels and sources are the word decoder's
                for (int k = 0; k < m; ++k) { G[2 * k] = 0; G[2 * k + 1] = 255; }
                const str_er_line_decode r = ld::decode_line(C.data(), G.data(), m, B.data(), pr[0], pr[1], chars.data(), src.data(), wor.data());
                CHECK(r.cost == d.cost && r.n_chars == d.n_chars && r.n_breaks == 0 && r.n_sub == d.n_sub && r.n_del == d.n_del && r.n_ins == d.n_ins);
                for (int k = 0; k < d.n_chars; ++k) CHECK(chars[k] == wc[k] && src[k] == (uint16_t)((ws[k] & 0x7F) | (ws[k] & 0x80 ? 0x8000 : 0)));
            }
        }
        str_er_line_decode r = ld::decode_line(C.data(), G.data(), m, B.data(), pr[0], pr[1], chars.data(), src.data(), wor.data());
        CHECK(r.cost == total && r.n_breaks == n_words - 1 && r.n_chars == (int)want.size());
        for (int k = 0; k < std::min(r.n_chars, (int)want.size()); ++k) CHECK(chars[k] == want[(size_t)k]);
        r = ld::decode_line(C.data(), F.data(), m, B.data(), pr[0], pr[1], chars.data(), src.data(), wor.data());
        CHECK(r.cost <= total + paid && r.cost == path_cost(C.data(), F.data(), m, B.data(), chars.data(), src.data(), r.n_chars, pr[0], pr[1]));
    }

    // the row limit and the bound of the contract
    {
        const int             n = 1025;
        std::vector<uint8_t>  C((size_t)n * 65, 255), B(wd::TABLE, 255), G((size_t)n * 2, 254), chars(3 * (size_t)n);
        std::vector<uint16_t> src(3 * (size_t)n);
        std::vector<int32_t>  wor((size_t)n, 7);
        str_er_line_decode r = ld::decode_line(C.data(), G.data(), n, B.data(), 0, 0, chars.data(), src.data(), wor.data());
        CHECK(r.cost == -1 && r.n_chars == 0 && r.n_breaks == 0 && r.n_sub == 0 && r.n_del == 0 && r.n_ins == 0 && chars[0] == 0xFF && src[3 * n - 1] == 0xFFFF && wor[n - 1] == -1);
        for (int i = 0; i < n; ++i) G[2 * i] = 255;
        r = ld::decode_line(C.data(), G.data(), 1024, B.data(), 0, 0, chars.data(), src.data(), wor.data());
        CHECK(r.cost == 1043202 && r.cost < wd::INF && r.n_breaks == 1023 && r.n_chars == 2047 && wor[1023] == 1023 && src[2046] == 1023 && src[2045] == (1023 | 0x4000));
        r = ld::decode_line(C.data(), G.data(), 0, B.data(), 0, 0, chars.data(), src.data(), wor.data());
        CHECK(r.cost == 255 && r.n_chars == 0);
    }

    // a dropped row between two breaks: an empty word, which costs B[E][E]
    {
        std::vector<uint8_t> C(3 * 65, 200), B(wd::TABLE, 9), G = {0, 0, 255, 0, 255, 0}, chars(9);
        uint16_t             src[9];
        int32_t              wor[3];
        C[0 * 65 + 64] = C[2 * 65 + 64] = 0;
        B[wd::E * wd::STATES + wd::E] = 1;
        const str_er_line_decode r = ld::decode_line(C.data(), G.data(), 3, B.data(), 0, 50, chars.data(), src, wor);
        CHECK(r.cost == 9 + 9 + 50 + 1 + 9 + 9 && r.n_breaks == 2 && r.n_del == 1 && r.n_chars == 4);
        CHECK(chars[0] == 64 && chars[1] == 65 && chars[2] == 65 && chars[3] == 64 && src[0] == 0 && src[1] == (1 | 0x4000) && src[2] == (2 | 0x4000) && src[3] == 2 && wor[0] == 0 && wor[1] == -1 && wor[2] == 2);
    }

    // the gap costs at their corners, and the argument checks
    {
        uint8_t p[2];
        const auto pair = [&](int64_t g, uint32_t colmax, int num, int den, int w) { ld::gap_pair(g, colmax, num, den, w, p); return p[0] * 1000 + p[1]; };
        CHECK(pair(3, 9, 1, 3, 16) == 16016 && pair(2, 9, 1, 3, 16) == 10022 && pair(1000, 9, 1, 3, 16) == 32000 && pair(3, 9, 1, 3, 0) == 0);
        CHECK(pair(3, 9, 1, 3, 127) == 127127 && pair(1 << 30, 1, 1, 65535, 127) == 254000 && pair(0, 9, 1, 3, 127) == 254 && pair(-4, 9, 1, 3, 127) == 254);
        CHECK(pair(1, 1, 1, 3, 16) == 32000 && pair(1, 16384, 65535, 1, 16) == 32);
        for (int w = 0; w <= 127; ++w)
            for (int x = 0; x <= 16; ++x) CHECK(w * x / 8 <= 254 && w * (16 - x) / 8 <= 254);
        str_er_line_run runs[3] = {{10, 20, 0, 9, 50, 0}, {23, 30, 0, 9, 50, 0}, {31, 40, 0, 9, 50, 1}};
        const int32_t   first[1] = {0}, n_of[1] = {3}, rr[4] = {0, 1, 1, 2}, n4[1] = {4};
        const uint32_t  colmax[1] = {9}, zero[1] = {0};
        uint8_t         g[8];
        CHECK(ld::gap_costs(runs, 3, nullptr, 3, first, n_of, colmax, 1, 1, 3, 16, g) && g[0] == 0 && g[1] == 255 && g[2] == 16 && g[3] == 16 && g[4] == 4 && g[5] == 28);
        CHECK(ld::gap_costs(runs, 3, rr, 4, first, n4, colmax, 1, 1, 3, 16, g) && g[4] == 0 && g[5] == 255 && g[6] == 4 && g[7] == 28);
        CHECK(!ld::gap_costs(runs, 2, nullptr, 3, first, n_of, colmax, 1, 1, 3, 16, g) && !ld::gap_costs(runs, 3, nullptr, 3, first, n_of, zero, 1, 1, 3, 16, g));
        const int32_t f2[2] = {0, 2}, n2[2] = {2, 1}, f_bad[2] = {0, 1}, n_neg[2] = {2, -1};
        CHECK(ld::lines_in_rows(3, f2, n2, 2) && !ld::lines_in_rows(2, f2, n2, 2) && !ld::lines_in_rows(3, f_bad, n2, 2) && !ld::lines_in_rows(3, f2, n_neg, 2));
        const uint8_t both[6] = {255, 255, 255, 255, 255, 255}, one[6] = {255, 255, 255, 0, 255, 255};
        CHECK(ld::gaps_ok(one, f2, n2, 2) && !ld::gaps_ok(both, f2, n2, 2) && ld::weight_ok(0) && ld::weight_ok(127) && !ld::weight_ok(128) && !ld::weight_ok(-1));
    }

    std::printf("%ld checks, %ld wrong\n", n_checks, n_wrong);
    return n_wrong ? 1 : 0;
}
