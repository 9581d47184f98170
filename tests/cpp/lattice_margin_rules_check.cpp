// lattice_margin_rules_check.cpp -- the rules of the lattice decoder's margins (csrc/lattice_margin_rules.h, the code the host entry point
// runs) on the CPU, under the host sanitizers: the edge marginals against an enumeration of every path on tables whose live part is 2
// characters, the identities of the contract on random words of the full alphabet, and its fixed vectors.  A program of its own;
// prints "<checks> checks, <wrong> wrong".
#include "../../scene-text-recognition_amd/csrc/lattice_margin_rules.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace ld = str_er_ld;
namespace rs = str_er_rs;
namespace wd = str_er_wd;

static long n_checks = 0, n_wrong = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++n_checks;                                                                  \
        if (!(cond)) { ++n_wrong; std::printf("line %d: %s\n", __LINE__, #cond); }   \
    } while (0)

static int B_at(const uint8_t *B, int a, int b) { return B[a * wd::STATES + b]; }

// a word of the runs 0 .. R-1 with the given cut counts; the pieces of the runs lie back to back
struct Word {
    std::vector<str_er_run_split> sp;
    std::vector<uint8_t>          rc, pc;
    int                           N = 0, n_edges = 0;
    explicit Word(const std::vector<int> &cuts)
    {
        int at = 0;
        for (const int k : cuts) {
            str_er_run_split s{};
            s.n_cuts = k; s.cut[0] = s.cut[1] = s.cut[2] = -1;
            s.first_piece = at; s.n_pieces = k > 0 ? (k + 1) * (k + 2) / 2 - 1 : 0;
            at += s.n_pieces;
            sp.push_back(s);
            N += k + 1; n_edges += (k + 1) * (k + 2) / 2;
        }
        rc.assign(sp.size() * 65, 255);
        pc.assign((size_t)at * 65 + 1, 255);
    }
    uint8_t *row(int r, int i, int j)
    {
        const int k = rs::piece_index(sp[r].n_cuts + 1, i, j);
        return k < 0 ? rc.data() + (size_t)r * 65 : pc.data() + ((size_t)sp[r].first_piece + (size_t)k) * 65;
    }
};

struct Out {
    str_er_lattice_decode d;
    str_er_lattice_margin r;
    uint8_t               chars[64], src[64], read[32], alt[32], cut_alt[32];
    str_er_split_part     parts[32];
    int32_t               read_margin[32], cut_margin[32], em[32 * 4];
    std::vector<int32_t>  M = std::vector<int32_t>(32 * 4 * 66);
};

static void run(Word &W, const uint8_t *B, int ins, int del, int split, Out &o, bool tables = true)
{
    const int R = (int)W.sp.size();
    o.d = ld::decode_word(W.sp.data(), W.rc.data(), W.pc.data(), 0, R, B, ins, del, split, o.chars, o.src, o.parts);
    o.r = ld::margins_word(W.sp.data(), W.rc.data(), W.pc.data(), 0, R, B, ins, del, split, o.chars, o.src, o.d.n_chars, o.parts, o.d.n_parts, o.read_margin,
                           o.cut_margin, o.read, o.alt, o.cut_alt, tables ? o.em : nullptr, tables ? o.M.data() : nullptr);
}

// every path over the live characters 0 .. n - 1 by brute force: per run a way through its atoms, per edge a drop or a reading, and behind
// either one inserted character that follows some character; best[node - 1][i][x]: the cheapest path that takes the edge from the local
// node i into that node and reads it as x (E: drops it)
struct Brute {
    Word          &W;
    const uint8_t *B;
    int            n, ins, del, split;
    int            edge_n[8], edge_i[8], how[8], depth;
    std::vector<int32_t> best;
    void walk(int r, int i, int node0, int prev, int32_t sofar)          // at the local node i of run r, whose local node 0 is node0
    {
        if (r == (int)W.sp.size()) {
            const int32_t s = sofar + B_at(B, prev, wd::E);
            for (int t = 0; t < depth; ++t) {
                int32_t &b = best[((edge_n[t] - 1) * 4 + edge_i[t]) * 66 + how[t]];
                b = b < 0 ? s : std::min(b, s);
            }
            return;
        }
        const int A = W.sp[r].n_cuts + 1;
        for (int j = i + 1; j <= A; ++j) {
            const uint8_t *row = W.row(r, i, j);
            const int32_t  pen = i > 0 ? split : 0;
            const auto     tail = [&](int32_t t, int p) {
                const auto next = [&](int32_t t2, int p2) { j == A ? walk(r + 1, 0, node0 + A, p2, t2) : walk(r, j, node0, p2, t2); };
                next(t, p);
                if (ins > 0 && p != wd::E)
                    for (int c = 0; c < n; ++c) next(t + B_at(B, p, c) + ins, c);
            };
            edge_n[depth] = node0 + j; edge_i[depth] = i;
            ++depth;
            if (del > 0) { how[depth - 1] = wd::E; tail(sofar + pen + del, prev); }
            for (int b = 0; b < n; ++b) { how[depth - 1] = b; tail(sofar + pen + B_at(B, prev, b) + row[b], b); }
            --depth;
        }
    }
};

// the identities of the contract on what margins_word left
static void identities(Word &W, const Out &o, int del)
{
    const int np = o.d.n_parts;
    CHECK(o.r.n_edges == W.n_edges && np >= 1);
    int edges = 0;
    for (int t = 0; t < 32 * 4; ++t) {
        const int32_t *M = o.M.data() + t * 66;
        if (o.em[t] < 0) {
            for (int x = 0; x < 66; ++x) CHECK(M[x] == -1);
            continue;
        }
        ++edges;
        int32_t lo = -1;
        for (int x = 0; x < 66; ++x) {
            CHECK(M[x] >= -1 && M[x] <= 41055 && (x < 65 ? M[x] >= 0 : (M[x] >= 0) == (del > 0)));
            if (M[x] >= 0 && (lo < 0 || M[x] < lo)) lo = M[x];
        }
        CHECK(lo == o.em[t] && lo >= o.d.cost);
    }
    CHECK(edges == W.n_edges);
    // every atom: the cheapest edge over it costs what the word costs
    int node0 = 0;
    for (const str_er_run_split &S : W.sp) {
        const int A = S.n_cuts + 1;
        for (int t = 0; t < A; ++t) {
            int32_t lo = -1;
            for (int i = 0; i <= t; ++i)
                for (int j = t + 1; j <= A; ++j) {
                    const int32_t v = o.em[(node0 + j - 1) * 4 + i];
                    if (lo < 0 || v < lo) lo = v;
                }
            CHECK(lo == o.d.cost);
        }
        node0 += A;
    }
    // the parts: a path from node 0 to node N; the margins against the tables
    int     n = 0, cut_at = -1, read_at = -1;
    int32_t cut_lo = -1, read_lo = -1;
    for (int k = 0; k < 32; ++k) {
        if (k >= np) {
            CHECK(o.read_margin[k] == -1 && o.cut_margin[k] == -1 && o.read[k] == 0xFF && o.alt[k] == 0xFF && o.cut_alt[k] == 0xFF);
            continue;
        }
        const int r = o.parts[k].run, A = W.sp[r].n_cuts + 1, kk = o.parts[k].piece < 0 ? -1 : o.parts[k].piece - W.sp[r].first_piece;
        int       off = 0, pi = -1, pj = -1;
        for (int q = 0; q < r; ++q) off += W.sp[q].n_cuts + 1;
        for (int i = 0; i < A; ++i)
            for (int j = i + 1; j <= A; ++j)
                if (rs::piece_index(A, i, j) == kk) { pi = i; pj = j; }
        CHECK(pi >= 0 && off + pi == n);
        n = off + pj;
        const int32_t *M = o.M.data() + ((n - 1) * 4 + pi) * 66;
        const int      x = o.read[k];
        int32_t        other = -1;
        int            other_at = -1;
        for (int y = 0; y < 66; ++y)
            if (y != x && M[y] >= 0 && (other < 0 || M[y] < other)) { other = M[y]; other_at = y; }
        CHECK(x <= 65 && M[x] == o.d.cost && o.read_margin[k] == other - o.d.cost && o.read_margin[k] >= 0 && o.alt[k] == other_at);
        int32_t cut = -1;
        int     ca = 0xFF;
        for (int i = 0; i < A; ++i)
            for (int j = i + 1; j <= A; ++j) {
                if ((i == pi && j == pj) || i >= pj || j <= pi) continue;
                const int32_t v = o.em[(off + j - 1) * 4 + i] - o.d.cost;
                if (cut < 0 || v < cut) { cut = v; ca = i | j << 4; }
            }
        CHECK(o.cut_margin[k] == cut && o.cut_alt[k] == ca && (cut < 0) == (A == 1));
        if (read_lo < 0 || o.read_margin[k] < read_lo) { read_lo = o.read_margin[k]; read_at = k; }
        if (cut >= 0 && (cut_lo < 0 || cut < cut_lo)) { cut_lo = cut; cut_at = k; }
    }
    CHECK(n == W.N);
    CHECK(o.r.read_margin == read_lo && o.r.read_part == read_at && o.r.read == o.read[read_at] && o.r.alt == o.alt[read_at]);
    CHECK(o.r.cut_margin == cut_lo && o.r.cut_part == cut_at && o.r.cut_alt == (cut_at < 0 ? -1 : o.cut_alt[cut_at]));
    for (int k = 0; k < o.d.n_chars; ++k)
        if (!(o.src[k] & 0x80)) CHECK(o.read[o.src[k]] == o.chars[k]);
}

int main()
{
    std::mt19937 rng(97531);
    const int    moves[6][3] = {{0, 0, 8}, {5, 0, 0}, {0, 7, 255}, {3, 4, 8}, {1, 1, 1}, {255, 255, 255}};
    Out          o;

    // a small alphabet inside the full one: the other characters cost 255 everywhere and the live costs stay below 40, so that no path
    // through a dead character can be the cheapest by a live reading (a dead character costs 255 or more on the way in and again on the
    // way out, a live one in its place at most 39 each way and 39 for its row); INS, DEL and SPLIT are kept at 30, 30 and 9 here
    const std::vector<std::vector<int>> shapes = {{0}, {1}, {2}, {3}, {0, 0}, {1, 1}, {0, 2}, {2, 0}, {1, 0, 1}};
    for (const auto &cuts : shapes)
        for (const auto &mv : moves)
            for (int rep = 0; rep < 4; ++rep) {
                const int n = 2, hi = rep % 2 ? 4 : 40, split = mv[2] == 255 ? 9 : mv[2];
                Word      W(cuts);
                std::vector<uint8_t> B(wd::TABLE, 255);
                for (int r = 0; r < (int)cuts.size(); ++r)
                    for (int i = 0; i <= cuts[r]; ++i)
                        for (int j = i + 1; j <= cuts[r] + 1; ++j)
                            for (int a = 0; a < n; ++a) W.row(r, i, j)[a] = (uint8_t)(rng() % hi);
                for (int a = 0; a <= n; ++a)
                    for (int b = 0; b <= n; ++b) B[(a == n ? wd::E : a) * wd::STATES + (b == n ? wd::E : b)] = (uint8_t)(rng() % hi);
                const int ins = std::min(mv[0], 30), del = std::min(mv[1], 30);
                run(W, B.data(), ins, del, split, o);
                Brute br{W, B.data(), n, ins, del, split, {}, {}, {}, 0, std::vector<int32_t>(32 * 4 * 66, -1)};
                br.walk(0, 0, 0, wd::E, 0);
                for (int t = 0; t < 32 * 4; ++t) {
                    for (int x = 0; x < n; ++x) CHECK(o.M[t * 66 + x] == br.best[t * 66 + x]);
                    CHECK(o.M[t * 66 + 65] == br.best[t * 66 + 65]);
                    CHECK((o.em[t] < 0) == (br.best[t * 66] < 0));
                }
                identities(W, o, del);
            }

    // random words on the full alphabet, dear and cheap tables, up to 32 atoms
    for (int it = 0; it < 120; ++it) {
        std::vector<int> cuts;
        int              N = 0;
        const int        want = 1 + (int)(rng() % 32);
        while (N < want) {
            const int k = std::min((int)(rng() % 4), want - N - 1);
            cuts.push_back(k);
            N += k + 1;
        }
        Word W(cuts);
        for (auto &v : W.rc) v = (uint8_t)(rng() % 10 == 0 ? rng() % 24 : 60 + rng() % 196);
        for (auto &v : W.pc) v = (uint8_t)(rng() % 10 == 0 ? rng() % 24 : (it % 3 ? 60 : 0) + rng() % 196);
        std::vector<uint8_t> B(wd::TABLE);
        for (auto &v : B) v = (uint8_t)(it % 2 ? rng() % 6 : rng() % 256);
        const auto &mv = moves[it % 6];
        run(W, B.data(), mv[0], mv[1], mv[2], o);
        CHECK(W.N == want && o.d.cost >= 0);
        identities(W, o, mv[1]);
        // without the tables the rest is the same
        Out p;
        run(W, B.data(), mv[0], mv[1], mv[2], p, false);
        CHECK(!std::memcmp(&p.r, &o.r, sizeof p.r) && !std::memcmp(p.read_margin, o.read_margin, sizeof p.read_margin) &&
              !std::memcmp(p.cut_margin, o.cut_margin, sizeof p.cut_margin) && !std::memcmp(p.read, o.read, 32) && !std::memcmp(p.alt, o.alt, 32) &&
              !std::memcmp(p.cut_alt, o.cut_alt, 32));
    }

    // the fixed vectors
    {
        std::vector<uint8_t> zero(wd::TABLE, 0), full(wd::TABLE, 255);
        // all zero, eight runs of three cuts: 32 nodes and 80 edges; every margin is 0, the reading 0, the alternative 1, the whole run
        // is the path and the atom (0, 1) the first other edge
        Word W(std::vector<int>(8, 3));
        std::fill(W.rc.begin(), W.rc.end(), 0); std::fill(W.pc.begin(), W.pc.end(), 0);
        run(W, zero.data(), 64, 64, 0, o);
        CHECK(o.d.cost == 0 && o.d.n_parts == 8 && o.r.read_margin == 0 && o.r.read_part == 0 && o.r.read == 0 && o.r.alt == 1);
        CHECK(o.r.cut_margin == 0 && o.r.cut_part == 0 && o.r.cut_alt == (0 | 1 << 4) && o.r.n_edges == 80);
        identities(W, o, 64);
        // everything at 255: the largest values there are
        std::fill(W.rc.begin(), W.rc.end(), 255); std::fill(W.pc.begin(), W.pc.end(), 255);
        run(W, full.data(), 0, 0, 255, o);
        CHECK(o.d.cost == 17 * 255 && o.r.read_margin == 0 && o.r.cut_margin == 3 * 255);
        identities(W, o, 0);
        run(W, full.data(), 255, 255, 255, o);
        CHECK(o.d.cost == 9 * 255 && o.r.read == 65 && o.r.alt == 0);
        identities(W, o, 255);
        int32_t top = 0;
        for (const int32_t v : o.M) top = std::max(top, v);
        CHECK(top <= 41055);
        // not decoded and no runs: the record of -1, nothing per part
        Word W33(std::vector<int>(33, 0)), W0(std::vector<int>{});
        for (Word *P : {&W33, &W0}) {
            run(*P, full.data(), 255, 255, 255, o);
            CHECK(o.r.read_margin == -1 && o.r.read_part == -1 && o.r.read == -1 && o.r.alt == -1 && o.r.cut_margin == -1 && o.r.cut_part == -1 && o.r.cut_alt == -1 &&
                  o.r.n_edges == 0);
            for (int k = 0; k < 32; ++k) CHECK(o.read_margin[k] == -1 && o.cut_margin[k] == -1 && o.read[k] == 0xFF && o.alt[k] == 0xFF && o.cut_alt[k] == 0xFF);
            for (int t = 0; t < 32 * 4; ++t) CHECK(o.em[t] == -1 && o.M[t * 66] == -1 && o.M[t * 66 + 65] == -1);
        }
        // an uncut word equals the word decoder's margins row for row
        Word U(std::vector<int>(9, 0));
        for (auto &v : U.rc) v = (uint8_t)(rng() % 256);
        std::vector<uint8_t> B(wd::TABLE);
        for (auto &v : B) v = (uint8_t)(rng() % 64);
        run(U, B.data(), 20, 30, 8, o);
        CHECK(o.r.cut_margin == -1 && o.r.cut_part == -1 && o.r.cut_alt == -1 && o.r.n_edges == 9);
        for (int k = 0; k < 9; ++k) CHECK(o.cut_margin[k] == -1 && o.cut_alt[k] == 0xFF);
        identities(U, o, 30);
    }

    std::printf("%ld checks, %ld wrong\n", n_checks, n_wrong);
    return n_wrong ? 1 : 0;
}
