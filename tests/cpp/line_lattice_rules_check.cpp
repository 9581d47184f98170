// line_lattice_rules_check.cpp -- the rules of the joint decode of a line over its runs' piece lattices (csrc/line_lattice_rules.h, the
// code the host entry point runs) on the CPU, under the host sanitizers: the recurrence against a plain restatement that walks every
// segmentation, every join / break choice, every string and every choice of moves on tables whose live part is 2 or 3 characters, the
// cost of the returned path recomputed from its labels, sources and parts, the identities of the contract against the rules of its
// parents (csrc/line_decode_rules.h, csrc/lattice_decode_rules.h), the line that is not decoded, the empty line, the bound and the node
// slots.  A program of its own; prints "<checks> checks, <wrong> wrong".
#include "../../scene-text-recognition_amd/csrc/line_lattice_rules.h"

#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

namespace wd = str_er_wd;
namespace ld = str_er_ld;
namespace rs = str_er_rs;

static long n_checks = 0, n_wrong = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++n_checks;                                                                  \
        if (!(cond)) { ++n_wrong; std::printf("line %d: %s\n", __LINE__, #cond); }   \
    } while (0)

static int B_at(const uint8_t *B, int a, int b) { return B[a * wd::STATES + b]; }

struct Line {
    std::vector<str_er_run_split> splits;
    std::vector<uint8_t>          runs, pieces, gaps;
    int                           R = 0, N = 0;
    const uint8_t *row(int r, int i, int j) const
    {
        const int k = rs::piece_index(splits[(size_t)r].n_cuts + 1, i, j);
        return k < 0 ? runs.data() + (size_t)r * 65 : pieces.data() + ((size_t)splits[(size_t)r].first_piece + (size_t)k) * 65;
    }
};

// a line of the given cut counts; fill(live) gives a byte of a row (live: one of the first n characters), g a gap byte
template <class F, class Gf>
static Line make_line(const std::vector<int> &cuts, int n, F fill, Gf g)
{
    Line L;
    L.R = (int)cuts.size();
    int at = 0;
    for (int k : cuts) {
        str_er_run_split S{};
        S.n_cuts = k; S.first_piece = at; S.n_pieces = rs::n_pieces(k);
        at += S.n_pieces;
        L.N += k + 1;
        L.splits.push_back(S);
    }
    L.runs.assign((size_t)std::max(L.R, 1) * 65, 255); L.pieces.assign((size_t)std::max(at, 1) * 65, 255); L.gaps.assign((size_t)std::max(L.R, 1) * 2, 0);
    for (int r = 0; r < L.R; ++r) {
        for (int a = 0; a < 65; ++a) L.runs[(size_t)r * 65 + a] = fill(a < n);
        L.gaps[2 * (size_t)r] = g(); L.gaps[2 * (size_t)r + 1] = g();
    }
    for (int p = 0; p < at; ++p)
        for (int a = 0; a < 65; ++a) L.pieces[(size_t)p * 65 + a] = fill(a < n);
    return L;
}

// the plain restatement: the cheapest way from the local node i of run r in the state prev (behind the run's gap where i = 0) to the
// end of the line, over the live characters 0 .. n - 1
static int32_t brute(const Line &L, int r, int i, int prev, const uint8_t *B, int n, int ins, int del, int split)
{
    if (r == L.R) return B_at(B, prev, wd::E);
    const int A = L.splits[(size_t)r].n_cuts + 1;
    int32_t   best = 1 << 30;
    const auto next = [&](int j, int p) -> int32_t {
        if (j < A) return brute(L, r, j, p, B, n, ins, del, split);
        if (r + 1 == L.R) return B_at(B, p, wd::E);
        int32_t       v = 1 << 30;
        const uint8_t J = L.gaps[2 * (size_t)(r + 1)], K = L.gaps[2 * (size_t)(r + 1) + 1];
        if (J != ld::OFF) v = std::min(v, J + brute(L, r + 1, 0, p, B, n, ins, del, split));
        if (K != ld::OFF) v = std::min(v, B_at(B, p, wd::E) + K + brute(L, r + 1, 0, wd::E, B, n, ins, del, split));
        return v;
    };
    for (int j = i + 1; j <= A; ++j) {
        const uint8_t *row = L.row(r, i, j);
        const int32_t  s = i > 0 ? split : 0;
        const auto tail = [&](int32_t sofar, int p) {
            best = std::min(best, sofar + next(j, p));
            if (ins > 0 && p != wd::E)
                for (int c = 0; c < n; ++c) best = std::min(best, sofar + B_at(B, p, c) + ins + next(j, c));
        };
        if (del > 0) tail(s + del, prev);
        for (int b = 0; b < n; ++b) tail(s + B_at(B, prev, b) + row[b], b);
    }
    return best;
}

struct Out {
    str_er_line_lattice_decode     r;
    std::vector<uint8_t>           chars;
    std::vector<uint16_t>          src;
    std::vector<str_er_split_part> parts;
    std::vector<int32_t>           wop;
};
static Out decode(const Line &L, int first, int n_of, const uint8_t *B, int ins, int del, int split)
{
    Out          o;
    const size_t N = (size_t)std::max<int64_t>(ld::word_nodes(L.splits.data(), first, std::max(n_of, 0)), 1);
    o.chars.assign(3 * N, 7); o.src.assign(3 * N, 7); o.parts.assign(N, str_er_split_part{7, 7}); o.wop.assign(N, 7);
    o.r = ld::decode_line_lattice(L.splits.data(), L.runs.data(), L.pieces.data(), L.gaps.data(), first, n_of, B, ins, del, split, o.chars.data(), o.src.data(), o.parts.data(),
                                  o.wop.data());
    return o;
}

// the cost of a returned path under the definition; false where the parts are no path or a blank stands where none can
static bool path_cost(const Line &L, const Out &o, const uint8_t *B, int ins, int del, int split, int32_t *cost)
{
    std::vector<int>  pi, pj, pr;
    std::vector<char> broken((size_t)std::max(L.R, 1), 0), used((size_t)std::max(o.r.n_parts, 1), 0);
    int32_t           s = 0;
    int               r = 0, at = 0;
    for (int k = 0; k < o.r.n_parts; ++k) {          // the parts are a path: each begins where the one before ended
        const str_er_split_part &P = o.parts[(size_t)k];
        if (P.run != r || r >= L.R) return false;
        const int A = L.splits[(size_t)r].n_cuts + 1;
        int       i = 0, j = A;
        if (P.piece >= 0) rs::piece_nodes(A, P.piece - L.splits[(size_t)r].first_piece, i, j);
        if (i != at) return false;
        pi.push_back(i); pj.push_back(j); pr.push_back(r);
        if (i > 0) s += split;
        at = j;
        if (at == A) { ++r; at = 0; }
    }
    if (r != L.R || at != 0) return false;
    int prev = wd::E, n_used = 0;
    for (int k = 0; k < o.r.n_chars; ++k) {
        const int a = o.chars[(size_t)k], p = o.src[(size_t)k] & 0x3FFF;
        if (p >= o.r.n_parts) return false;
        s += B_at(B, prev, a);
        if (o.src[(size_t)k] & ld::SRC_BREAK) {
            if (a != wd::E || pi[(size_t)p] != 0 || pr[(size_t)p] == 0 || broken[(size_t)pr[(size_t)p]]) return false;
            s += L.gaps[2 * (size_t)pr[(size_t)p] + 1]; broken[(size_t)pr[(size_t)p]] = 1;
        } else if (o.src[(size_t)k] & ld::SRC_INS) s += ins;
        else {
            if (used[(size_t)p]) return false;
            s += L.row(pr[(size_t)p], pi[(size_t)p], pj[(size_t)p])[a]; used[(size_t)p] = 1; ++n_used;
        }
        prev = a;
    }
    for (int q = 1; q < L.R; ++q)
        if (!broken[(size_t)q]) s += L.gaps[2 * (size_t)q];
    *cost = s + B_at(B, prev, wd::E) + del * (o.r.n_parts - n_used);
    return true;
}

int main()
{
    std::mt19937 rng(8642);
    const int    pairs[4][2] = {{0, 0}, {64, 0}, {0, 64}, {64, 64}};

    // small alphabets inside the full one: the other characters cost 255 everywhere and the live costs stay below hi <= 40, so that no
    // path through a dead character can win; the moves scaled to the live costs
    const std::vector<std::vector<int>> shapes = {{}, {0}, {1}, {2}, {0, 0}, {0, 1}, {1, 0}, {2, 0}, {0, 2}, {1, 1}, {2, 1}, {1, 2}, {2, 2}, {0, 0, 0}, {1, 0, 1}, {0, 2, 0}, {1, 1, 1}, {3}, {3, 0}};
    for (int n = 2; n <= 3; ++n)
        for (const auto &cuts : shapes) {
            int N = 0;
            for (int k : cuts) N += k + 1;
            if (n == 3 && N > 4) continue;
            for (const auto &pr : pairs)
                for (int rep = 0; rep < (N > 4 ? 3 : 8); ++rep) {
                    const int hi = rep % 2 ? 4 : 40, ins = pr[0] * hi / 256, del = pr[1] * hi / 256, split = (rep % 3) * hi / 8;
                    Line L = make_line(cuts, n, [&](bool live) { return (uint8_t)(live ? rng() % hi : 255); }, [&] { return (uint8_t)(rng() % hi); });
                    for (int r = 0; r < L.R; ++r)
                        if (rng() % 5 == 0) L.gaps[2 * (size_t)r + rng() % 2] = 255;
                    std::vector<uint8_t> B(wd::TABLE, 255);
                    for (int a = 0; a <= n; ++a)
                        for (int b = 0; b <= n; ++b) B[(a == n ? wd::E : a) * wd::STATES + (b == n ? wd::E : b)] = (uint8_t)(rng() % hi);
                    const Out o = decode(L, 0, L.R, B.data(), ins, del, split);
                    int32_t   pc = -1;
                    CHECK(o.r.cost == brute(L, 0, 0, wd::E, B.data(), n, ins, del, split));
                    CHECK(path_cost(L, o, B.data(), ins, del, split, &pc) && pc == o.r.cost);
                    CHECK(o.r.n_sub + o.r.n_ins + o.r.n_breaks == o.r.n_chars && o.r.n_sub + o.r.n_del == o.r.n_parts && o.r.n_chars <= std::max(0, 3 * N - 1));
                    CHECK(o.r.n_parts >= L.R && o.r.n_parts <= N && o.r.first_part == 0 && (ins > 0 || o.r.n_ins == 0) && (del > 0 || o.r.n_del == 0));
                    for (int k = 0; k < 3 * N; ++k)
                        CHECK(k < o.r.n_chars ? (o.chars[(size_t)k] < n || o.chars[(size_t)k] == wd::E) : (o.chars[(size_t)k] == 0xFF && o.src[(size_t)k] == 0xFFFF));
                    int at = 0;
                    for (int k = 0; k < N; ++k) {
                        if (k >= o.r.n_parts) { CHECK(o.parts[(size_t)k].run == -1 && o.parts[(size_t)k].piece == -1 && o.wop[(size_t)k] == -1); continue; }
                        CHECK(o.wop[(size_t)k] == -1 || (o.wop[(size_t)k] >= at && o.wop[(size_t)k] <= o.r.n_breaks));
                        if (o.wop[(size_t)k] >= 0) at = o.wop[(size_t)k];
                    }
                }
        }

    // the identities on the full alphabet
    for (int it = 0; it < 160; ++it) {
        const auto &pr = pairs[it % 4];
        const int   split = (it % 3) * 100, R = (int)(rng() % 9);
        std::vector<int> cuts((size_t)R);
        for (auto &k : cuts) k = it % 5 == 0 ? 0 : (int)(rng() % 4);
        Line L = make_line(cuts, 65, [&](bool) { return (uint8_t)(rng() % 10 == 0 ? rng() % 24 : 60 + rng() % 196); }, [&] { return (uint8_t)(rng() % 255); });
        std::vector<uint8_t> B(wd::TABLE);
        for (auto &v : B) v = (uint8_t)(rng() % (it % 2 ? 256 : 6));
        const Out free_gaps = decode(L, 0, R, B.data(), pr[0], pr[1], split);
        int32_t   pc = -1;
        CHECK(path_cost(L, free_gaps, B.data(), pr[0], pr[1], split, &pc) && pc == free_gaps.r.cost);
        {          // (4) never worse than the line decoder on the runs' rows; (1) without cuts it is the line decoder, byte for byte
            const size_t          m = (size_t)std::max(R, 1);
            std::vector<uint8_t>  chars(3 * m);
            std::vector<uint16_t> src(3 * m);
            std::vector<int32_t>  wor(m);
            const str_er_line_decode d = ld::decode_line(L.runs.data(), L.gaps.data(), R, B.data(), pr[0], pr[1], chars.data(), src.data(), wor.data());
            CHECK(free_gaps.r.cost <= d.cost);
            if (it % 5 == 0) {
                const str_er_line_lattice_decode &r = free_gaps.r;
                CHECK(r.cost == d.cost && r.n_chars == d.n_chars && r.n_breaks == d.n_breaks && r.n_sub == d.n_sub && r.n_del == d.n_del && r.n_ins == d.n_ins && r.n_parts == R);
                for (int k = 0; k < 3 * R; ++k) CHECK(free_gaps.chars[(size_t)k] == chars[(size_t)k] && free_gaps.src[(size_t)k] == src[(size_t)k]);
                for (int k = 0; k < R; ++k) CHECK(free_gaps.wop[(size_t)k] == wor[(size_t)k] && free_gaps.parts[(size_t)k].run == k && free_gaps.parts[(size_t)k].piece == -1);
            }
        }
        // (3) a segmentation into words of at most 8 runs forced by its gaps, every word gap at a cost of its own; with one word that is (2)
        int32_t                        total = 0;
        std::vector<uint8_t>           want;
        std::vector<str_er_split_part> want_parts;
        int                            n_words = 0;
        for (int at = 0; at < R; ++n_words) {
            const int len = std::min(R - at, 1 + (int)(rng() % 8));
            uint8_t           wc[64], ws[64];
            str_er_split_part wp[32];
            const str_er_lattice_decode d = ld::decode_word(L.splits.data(), L.runs.data(), L.pieces.data(), at, len, B.data(), pr[0], pr[1], split, wc, ws, wp);
            CHECK(d.cost >= 0);
            total += d.cost;
            if (at > 0) { want.push_back(65); total += L.gaps[2 * (size_t)at + 1]; }          // (a gap byte here is below 255: on)
            want.insert(want.end(), wc, wc + d.n_chars);
            want_parts.insert(want_parts.end(), wp, wp + d.n_parts);
            for (int k = 0; k < len; ++k) L.gaps[2 * (size_t)(at + k)] = k ? 0 : 255;
            for (int k = 1; k < len; ++k) L.gaps[2 * (size_t)(at + k) + 1] = 255;
            at += len;
        }
        const Out forced = decode(L, 0, R, B.data(), pr[0], pr[1], split);
        CHECK(forced.r.cost == (R ? total : B_at(B.data(), wd::E, wd::E)) && forced.r.n_breaks == std::max(n_words - 1, 0) && forced.r.n_chars == (int)want.size());
        CHECK(forced.r.n_parts == (int)want_parts.size());
        for (int k = 0; k < std::min(forced.r.n_chars, (int)want.size()); ++k) CHECK(forced.chars[(size_t)k] == want[(size_t)k]);
        for (int k = 0; k < std::min(forced.r.n_parts, (int)want_parts.size()); ++k)
            CHECK(forced.parts[(size_t)k].run == want_parts[(size_t)k].run && forced.parts[(size_t)k].piece == want_parts[(size_t)k].piece);
    }

    // a window inside the table: the line of the runs 2 .. 4 of 6 reads its own gap pairs and names its own runs
    {
        Line L = make_line({1, 0, 2, 0, 3, 1}, 65, [&](bool) { return (uint8_t)(rng() % 10 == 0 ? rng() % 24 : 60 + rng() % 196); }, [&] { return (uint8_t)(rng() % 255); });
        std::vector<uint8_t> B(wd::TABLE);
        for (auto &v : B) v = (uint8_t)(rng() % 6);
        const Out o = decode(L, 2, 3, B.data(), 20, 30, 8);
        Line M = make_line({2, 0, 3}, 65, [](bool) { return (uint8_t)0; }, [] { return (uint8_t)0; });
        std::copy(L.runs.begin() + 2 * 65, L.runs.begin() + 5 * 65, M.runs.begin());
        std::copy(L.gaps.begin() + 4, L.gaps.begin() + 10, M.gaps.begin());
        std::copy(L.pieces.begin() + (size_t)L.splits[2].first_piece * 65, L.pieces.begin() + (size_t)L.splits[5].first_piece * 65, M.pieces.begin());
        const Out m = decode(M, 0, 3, B.data(), 20, 30, 8);
        CHECK(o.r.cost == m.r.cost && o.r.n_chars == m.r.n_chars && o.r.n_parts == m.r.n_parts && o.chars == m.chars && o.src == m.src && o.wop == m.wop);
        for (int k = 0; k < o.r.n_parts; ++k)
            CHECK(o.parts[(size_t)k].run == m.parts[(size_t)k].run + 2 &&
                  (m.parts[(size_t)k].piece < 0 ? o.parts[(size_t)k].piece == -1 : o.parts[(size_t)k].piece == m.parts[(size_t)k].piece + L.splits[2].first_piece));
    }

    // the line that is not decoded, the bound of the contract at 1024 runs of four atoms, and the empty line
    {
        const int        R = 1025;
        std::vector<int> cuts((size_t)R, 3);
        Line L = make_line(cuts, 65, [](bool) { return (uint8_t)255; }, [] { return (uint8_t)254; });
        std::vector<uint8_t> B(wd::TABLE, 255);
        Out o = decode(L, 0, R, B.data(), 0, 0, 255);
        CHECK(o.r.cost == -1 && o.r.n_chars == 0 && o.r.n_breaks == 0 && o.r.n_sub == 0 && o.r.n_del == 0 && o.r.n_ins == 0 && o.r.n_parts == 0 && o.r.first_part == 0);
        CHECK(o.chars[0] == 0xFF && o.src[3 * 4 * (size_t)R - 1] == 0xFFFF && o.parts[0].run == -1 && o.parts[4 * (size_t)R - 1].piece == -1 && o.wop[4 * (size_t)R - 1] == -1);
        for (int r = 0; r < R; ++r) L.gaps[2 * (size_t)r] = 255;
        o = decode(L, 0, 1024, B.data(), 0, 0, 255);
        CHECK(o.r.cost == 1043202 && o.r.cost < wd::INF && o.r.n_breaks == 1023 && o.r.n_chars == 2047 && o.r.n_parts == 1024 && o.wop[1023] == 1023);
        CHECK(o.src[2046] == 1023 && o.src[2045] == (1023 | 0x4000) && o.parts[1023].run == 1023 && o.parts[1023].piece == -1 && o.parts[1024].run == -1 && o.chars[2047] == 0xFF);
        o = decode(L, 1, 1024, B.data(), 255, 255, 255);          // (with every move at its dearest the values still stay inside the keys: no overflow under UBSan)
        CHECK(o.r.cost > 0 && o.r.cost < wd::INF && o.r.n_parts >= 1024);
        o = decode(L, 5, 0, B.data(), 0, 0, 255);
        CHECK(o.r.cost == 255 && o.r.n_chars == 0 && o.r.n_parts == 0 && o.chars[0] == 7 && o.parts[0].run == 7);          // (nothing written past its empty slices)
        o = decode(L, 5, -3, B.data(), 0, 0, 255);
        CHECK(o.r.cost == 255 && o.r.n_parts == 0);
    }

    // the node slots and the argument checks
    {
        str_er_run_split S[4] = {};
        S[0].n_cuts = 3; S[1].n_cuts = 0; S[2].n_cuts = 2; S[3].n_cuts = 1;
        std::vector<int32_t> slots;
        CHECK(ld::ll_node_slots(S, 4, slots) && slots.size() == 5 && slots[0] == 0 && slots[1] == 4 && slots[2] == 5 && slots[3] == 8 && slots[4] == 10);
        CHECK(ld::ll_node_slots(S, 0, slots) && slots.size() == 1 && slots[0] == 0);
        const int32_t f2[2] = {0, 2}, n2[2] = {2, 1}, f_bad[2] = {0, 1}, n_neg[2] = {2, -1};
        CHECK(ld::lines_in_rows(3, f2, n2, 2) && !ld::lines_in_rows(2, f2, n2, 2) && !ld::lines_in_rows(3, f_bad, n2, 2) && !ld::lines_in_rows(3, f2, n_neg, 2));
        const uint8_t both[6] = {255, 255, 255, 255, 255, 255}, one[6] = {255, 255, 255, 0, 255, 255};
        CHECK(ld::ll_gaps_ok(one, f2, n2, 2) && !ld::ll_gaps_ok(both, f2, n2, 2));
        CHECK(ld::params_ok(0, 0, 0) && ld::params_ok(255, 255, 255) && !ld::params_ok(0, 0, 256) && !ld::params_ok(-1, 0, 0));
    }

    std::printf("%ld checks, %ld wrong\n", n_checks, n_wrong);
    return n_wrong ? 1 : 0;
}
