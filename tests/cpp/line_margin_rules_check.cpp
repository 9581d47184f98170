// line_margin_rules_check.cpp -- the rules of the line decoder's margins (csrc/line_margin_rules.h, the code the host entry point runs)
// on the CPU, under the host sanitizers: every marginal against an enumeration of every path on tables whose live part is 2 or 3
// characters, the two "the reading attains cost" statements, the identities of the contract against the word margins' rules
// (csrc/word_margin_rules.h) and against a second decode with the decided move off, the row limit and its bound.  A program of its own;
// prints "<checks> checks, <wrong> wrong".
#include "../../scene-text-recognition_amd/csrc/line_margin_rules.h"
#include "../../scene-text-recognition_amd/csrc/word_margin_rules.h"

#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

namespace wd = str_er_wd;
namespace ld = str_er_ld;
namespace lm = str_er_lm;

static long n_checks = 0, n_wrong = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++n_checks;                                                                  \
        if (!(cond)) { ++n_wrong; std::printf("line %d: %s\n", __LINE__, #cond); }   \
    } while (0)

static int B_at(const uint8_t *B, int a, int b) { return B[a * wd::STATES + b]; }

// every path over the live characters 0 .. n - 1, as line_decode_rules_check.cpp's brute: what row i does (read as b: b, dropped: 65)
// goes to did[i], the move of the gap in front of it to gap[i], and a finished path lowers the minima of all it did
struct Brute {
    const uint8_t *C, *G, *B;
    int            m, n, ins, del;
    std::vector<int>     did, gap;
    std::vector<int32_t> M;          // m x 68, -1: none

    void end(int32_t s, int prev)
    {
        s += B_at(B, prev, wd::E);
        for (int i = 0; i < m; ++i) {
            int32_t &a = M[(size_t)i * lm::MARGINALS + did[i]];
            if (a < 0 || s < a) a = s;
            if (i >= 1) {
                int32_t &g = M[(size_t)i * lm::MARGINALS + (gap[i] ? lm::BREAK : lm::JOIN)];
                if (g < 0 || s < g) g = s;
            }
        }
    }
    void go(int i, int32_t s, int prev)
    {
        if (i == m) { end(s, prev); return; }
        const auto row = [&](int32_t s0, int p0) {
            const auto tail = [&](int32_t s1, int p) {
                go(i + 1, s1, p);
                if (ins > 0 && p != wd::E)
                    for (int c = 0; c < n; ++c) go(i + 1, s1 + B_at(B, p, c) + ins, c);
            };
            if (del > 0) { did[i] = wd::E; tail(s0 + del, p0); }
            for (int b = 0; b < n; ++b) { did[i] = b; tail(s0 + B_at(B, p0, b) + C[i * 65 + b], b); }
        };
        if (i == 0) row(s, prev);
        else {
            if (G[2 * i] != ld::OFF) { gap[i] = 0; row(s + G[2 * i], prev); }
            if (G[2 * i + 1] != ld::OFF) { gap[i] = 1; row(s + B_at(B, prev, wd::E) + G[2 * i + 1], wd::E); }
        }
    }
};

struct Line {
    str_er_line_decode    dec;
    str_er_line_margin    rec;
    std::vector<uint8_t>  chars, rr, ra, gv;
    std::vector<uint16_t> src;
    std::vector<int32_t>  wor, rm, gm, mg;
};

static Line run(const uint8_t *C, const uint8_t *G, int m, const uint8_t *B, int ins, int del)
{
    Line         L;
    const size_t mm = (size_t)std::max(m, 1);
    L.chars.resize(3 * mm); L.src.resize(3 * mm); L.wor.resize(mm);
    L.rr.assign(mm, 7); L.ra.assign(mm, 7); L.gv.assign(mm, 7); L.rm.assign(mm, 7); L.gm.assign(mm, 7); L.mg.assign(mm * lm::MARGINALS, 7);
    L.dec = ld::decode_line(C, G, m, B, ins, del, L.chars.data(), L.src.data(), L.wor.data());
    L.rec = lm::margins_line(C, G, m, B, ins, del, L.chars.data(), L.src.data(), L.dec.n_chars, L.rm.data(), L.rr.data(), L.ra.data(), L.gm.data(), L.gv.data(), L.mg.data());
    return L;
}

int main()
{
    std::mt19937 rng(1320);
    const int    pairs[6][2] = {{0, 0}, {5, 0}, {0, 7}, {3, 4}, {1, 1}, {255, 255}};

    // small alphabets inside the full one: the other characters cost 255 everywhere and the live costs stay below 40, so that no path
    // through a dead character can be the cheapest of anything the live part does
    for (int n = 2; n <= 3; ++n)
        for (int m = 1; m <= 4; ++m)
            for (const auto &pr : pairs)
                for (int rep = 0; rep < (m == 4 ? 3 : 10); ++rep) {
                    const int            hi = rep % 2 ? 4 : 40, ins = pr[0], del = pr[1];
                    std::vector<uint8_t> C((size_t)m * 65, 255), B(wd::TABLE, 255), G((size_t)m * 2);
                    for (int i = 0; i < m; ++i) {
                        for (int a = 0; a < n; ++a) C[i * 65 + a] = (uint8_t)(rng() % hi);
                        G[2 * i] = (uint8_t)(rng() % hi); G[2 * i + 1] = (uint8_t)(rng() % hi);
                        if (rng() % 4 == 0) G[2 * i + rng() % 2] = 255;
                    }
                    for (int a = 0; a <= n; ++a)
                        for (int b = 0; b <= n; ++b) B[(a == n ? wd::E : a) * wd::STATES + (b == n ? wd::E : b)] = (uint8_t)(rng() % hi);
                    const Line L = run(C.data(), G.data(), m, B.data(), ins, del);
                    Brute      E{C.data(), G.data(), B.data(), m, n, ins, del, std::vector<int>((size_t)m), std::vector<int>((size_t)m),
                            std::vector<int32_t>((size_t)m * lm::MARGINALS, -1)};
                    E.go(0, 0, wd::E);
                    for (int i = 0; i < m; ++i) {
                        const int32_t *got = L.mg.data() + (size_t)i * lm::MARGINALS, *want = E.M.data() + (size_t)i * lm::MARGINALS;
                        for (int k = 0; k < n; ++k) CHECK(got[k] == want[k]);
                        for (int k = wd::E; k < lm::MARGINALS; ++k) CHECK(got[k] == want[k]);
                        // the readings attain cost; the margins are those of the marginals
                        CHECK(L.rr[i] <= wd::E && got[L.rr[i]] == L.dec.cost && L.rm[i] >= 0 && L.ra[i] != L.rr[i] && got[L.ra[i]] == L.dec.cost + L.rm[i]);
                        if (i == 0) CHECK(L.gv[0] == 0xFF && L.gm[0] == -1 && got[lm::JOIN] == -1 && got[lm::BREAK] == -1);
                        else {
                            CHECK(L.gv[i] <= 1 && got[lm::JOIN + L.gv[i]] == L.dec.cost);
                            const int32_t other = got[lm::JOIN + 1 - L.gv[i]];
                            CHECK(L.gm[i] == (other < 0 ? -1 : other - L.dec.cost) && (other >= 0) == (G[2 * i + 1 - L.gv[i]] != ld::OFF));
                        }
                    }
                    int32_t rmin = 1 << 30, gmin = -1;
                    for (int i = 0; i < m; ++i) { rmin = std::min(rmin, L.rm[i]); if (L.gm[i] >= 0 && (gmin < 0 || L.gm[i] < gmin)) gmin = L.gm[i]; }
                    CHECK(L.rec.read_margin == rmin && L.rec.gap_margin == gmin && L.rec.margin == (gmin >= 0 && gmin < rmin ? gmin : rmin));
                    CHECK(L.rm[L.rec.row] == rmin && L.rec.read == L.rr[L.rec.row] && L.rec.alt == L.ra[L.rec.row]);
                    CHECK(gmin < 0 ? (L.rec.gap == -1 && L.rec.gap_move == -1) : (L.gm[L.rec.gap] == gmin && L.rec.gap_move == L.gv[L.rec.gap]));
                }

    // the identities on the full alphabet
    for (int it = 0; it < 90; ++it) {
        const auto &pr = pairs[it % 6];
        int        lengths[5], n_words = 1 + (int)(rng() % 5), m = 0;
        for (int w = 0; w < n_words; ++w) { lengths[w] = 1 + (int)(rng() % 8); m += lengths[w]; }
        std::vector<uint8_t> C((size_t)m * 65), B(wd::TABLE), G((size_t)m * 2), F((size_t)m * 2);
        for (auto &v : C) v = (uint8_t)(rng() % 10 == 0 ? rng() % 24 : 60 + rng() % 196);
        for (auto &v : B) v = (uint8_t)(rng() % (it % 3 ? 256 : 6));
        for (auto &v : F) v = (uint8_t)(rng() % (it % 2 ? 255 : 8));
        for (int w = 0, at = 0; w < n_words; at += lengths[w], ++w)
            for (int k = 0; k < lengths[w]; ++k) { G[2 * (at + k)] = k ? 0 : 255; G[2 * (at + k) + 1] = k ? 255 : 0; }
        // (2), and with one word (1): the row outputs are the word margins', the marginals the word's plus the other words' costs
        const Line L = run(C.data(), G.data(), m, B.data(), pr[0], pr[1]);
        for (int w = 0, at = 0; w < n_words; at += lengths[w], ++w) {
            uint8_t wc[64], ws[64], rr[32], ra[32];
            int32_t rm[32], mg[32 * wd::MARGINALS];
            const str_er_word_decode d = wd::decode_word(C.data() + (size_t)at * 65, lengths[w], B.data(), pr[0], pr[1], wc, ws);
            wd::margins_word(C.data() + (size_t)at * 65, lengths[w], B.data(), pr[0], pr[1], wc, ws, d.n_chars, rm, rr, ra, mg);
            for (int k = 0; k < lengths[w]; ++k) {
                CHECK(L.rm[at + k] == rm[k] && L.rr[at + k] == rr[k] && L.ra[at + k] == ra[k] && L.gm[at + k] == -1);
                CHECK(L.gv[at + k] == (at + k == 0 ? 0xFF : k == 0 ? 1 : 0));
                for (int x = 0; x < wd::MARGINALS; ++x)
                    CHECK(L.mg[(size_t)(at + k) * lm::MARGINALS + x] == (mg[k * wd::MARGINALS + x] < 0 ? -1 : mg[k * wd::MARGINALS + x] + L.dec.cost - d.cost));
            }
        }
        CHECK(L.rec.gap_margin == -1 && L.rec.gap == -1 && L.rec.gap_move == -1 && L.rec.margin == L.rec.read_margin);
        // (3): with the decided move of a gap off, the line costs cost + the gap's margin
        const Line Q = run(C.data(), F.data(), m, B.data(), pr[0], pr[1]);
        for (int i = 1; i < m; ++i) {
            if (Q.gm[i] < 0) continue;
            std::vector<uint8_t> F2 = F;
            F2[2 * i + Q.gv[i]] = 255;
            CHECK(run(C.data(), F2.data(), m, B.data(), pr[0], pr[1]).dec.cost == Q.dec.cost + Q.gm[i]);
        }
    }

    // the row limit and the bound of the contract
    {
        const int            n = 1025;
        std::vector<uint8_t> C((size_t)n * 65, 255), B(wd::TABLE, 255), G((size_t)n * 2, 254);
        Line L = run(C.data(), G.data(), n, B.data(), 0, 0);
        CHECK(L.rec.margin == -1 && L.rec.read_margin == -1 && L.rec.row == -1 && L.rec.read == -1 && L.rec.alt == -1 && L.rec.gap_margin == -1 && L.rec.gap == -1 && L.rec.gap_move == -1);
        CHECK(L.rm[n - 1] == -1 && L.rr[0] == 0xFF && L.ra[n - 1] == 0xFF && L.gm[0] == -1 && L.gv[n - 1] == 0xFF && L.mg[(size_t)n * lm::MARGINALS - 1] == -1);
        L = run(C.data(), G.data(), 0, B.data(), 0, 0);
        CHECK(L.rec.margin == -1 && L.rec.gap_move == -1 && L.rm[0] == 7);          // (no rows: nothing is written)
        for (int i = 0; i < n; ++i) G[2 * i] = 255;
        L = run(C.data(), G.data(), 1024, B.data(), 0, 0);
        CHECK(L.dec.cost == 1043202 && *std::max_element(L.mg.begin(), L.mg.begin() + 1024 * lm::MARGINALS) == 1043202 && L.rec.margin == 0 && L.rec.alt == 1 && L.rec.gap_margin == -1);
        for (int i = 0; i < n; ++i) G[2 * i] = 254;
        L = run(C.data(), G.data(), 1024, B.data(), 0, 0);
        CHECK(L.dec.cost == 510 + (255 + 255 + 254) * 1023 + 255 && L.gm[1] == 255 && L.gv[1] == 0 && L.rec.gap_margin == 255 && L.rec.gap == 1);
    }

    std::printf("%ld checks, %ld wrong\n", n_checks, n_wrong);
    return n_wrong ? 1 : 0;
}
