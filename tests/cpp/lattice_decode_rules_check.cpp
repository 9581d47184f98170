// lattice_decode_rules_check.cpp -- the rules of the joint decode over the piece lattice (csrc/lattice_decode_rules.h, the code the host
// entry point runs) on the CPU, under the host sanitizers: the recurrence against an enumeration of every path, string and choice of
// moves on tables whose live part is 2 or 3 characters, the cost of the returned path and string recomputed from its labels, sources and
// parts, words without cuts against the word decoder's rules, hand-made words (N = 0, 1, 32, 33, all-equal rows, maximal values), and
// the rules of STR_ER_WANT_LATTICE_DECODE in check_stages (csrc/stage_rules.h).  A program of its own; prints "<checks> checks, <wrong> wrong".
#include "../../scene-text-recognition_amd/csrc/lattice_decode_rules.h"
#include "../../scene-text-recognition_amd/csrc/stage_rules.h"

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

// a word: its split records and the rows of its runs and pieces
struct Word {
    std::vector<str_er_run_split> splits;
    std::vector<uint8_t>          runs, pieces;
    const uint8_t *row(int r, int i, int j) const
    {
        const int k = rs::piece_index(splits[(size_t)r].n_cuts + 1, i, j);
        return k < 0 ? &runs[(size_t)r * 65] : &pieces[((size_t)splits[(size_t)r].first_piece + (size_t)k) * 65];
    }
    int nodes() const { int n = 0; for (const auto &s : splits) n += s.n_cuts + 1; return n; }
};

template <class Fill> static Word make_word(const std::vector<int> &cuts, Fill fill)
{
    Word w;
    int  at = 0;
    for (const int k : cuts) {
        w.splits.push_back(str_er_run_split{k, {-1, -1, -1}, 0, at, rs::n_pieces(k), 0});
        at += rs::n_pieces(k);
    }
    w.runs.resize(std::max<size_t>(cuts.size(), 1) * 65);
    w.pieces.resize(std::max(at, 1) * 65);
    for (auto &v : w.runs) v = fill();
    for (auto &v : w.pieces) v = fill();
    return w;
}

// the cheapest way from the local node i of run r with the last character prev, over the live characters 0 .. n - 1, by brute force: per
// edge a drop or a reading, and behind either one inserted character that follows some character
static int32_t brute(const Word &w, int r, int i, int prev, const uint8_t *B, int n, int ins, int del, int split)
{
    if (r == (int)w.splits.size()) return B_at(B, prev, wd::E);
    const int A = w.splits[(size_t)r].n_cuts + 1;
    int32_t   best = 1 << 30;
    for (int j = i + 1; j <= A; ++j) {
        const uint8_t *row = w.row(r, i, j);
        const int      s = i > 0 ? split : 0, r2 = j == A ? r + 1 : r, i2 = j == A ? 0 : j;
        const auto tail = [&](int32_t sofar, int p) {
            best = std::min(best, sofar + brute(w, r2, i2, p, B, n, ins, del, split));
            if (ins > 0 && p != wd::E)
                for (int c = 0; c < n; ++c) best = std::min(best, sofar + B_at(B, p, c) + ins + brute(w, r2, i2, c, B, n, ins, del, split));
        };
        if (del > 0) tail(del + s, prev);
        for (int b = 0; b < n; ++b) tail(B_at(B, prev, b) + row[b] + s, b);
    }
    return best;
}

// the cost of a returned path and string under the definition; -1 where the parts are no path through the lattice
static int32_t path_cost(const Word &w, const uint8_t *B, const uint8_t *chars, const uint8_t *src, const str_er_lattice_decode &d, const str_er_split_part *parts,
                         int ins, int del, int split)
{
    std::vector<const uint8_t *> rows;
    int32_t s = 0;
    int     run = 0, node = 0;
    for (int t = 0; t < d.n_parts; ++t) {
        const str_er_split_part &P = parts[t];
        if (P.run != run) return -1;
        const int A = w.splits[(size_t)run].n_cuts + 1;
        int       i = 0, j = A;
        if (P.piece >= 0) rs::piece_nodes(A, P.piece - w.splits[(size_t)run].first_piece, i, j);
        if (i != node) return -1;
        rows.push_back(w.row(run, i, j));
        s += i > 0 ? split : 0;
        node = j == A ? 0 : j;
        run += j == A;
    }
    if (run != (int)w.splits.size() || node != 0) return -1;
    int prev = wd::E, used = 0;
    for (int k = 0; k < d.n_chars; ++k) {
        s += B_at(B, prev, chars[k]);
        if (src[k] & 0x80) s += ins;
        else { s += rows[(size_t)(src[k] & 0x7F)][chars[k]]; ++used; }
        if ((src[k] & 0x7F) >= d.n_parts) return -1;
        prev = chars[k];
    }
    return s + B_at(B, prev, wd::E) + del * (d.n_parts - used);
}

static str_er_lattice_decode decode(const Word &w, const uint8_t *B, int ins, int del, int split, uint8_t *chars, uint8_t *src, str_er_split_part *parts)
{
    return ld::decode_word(w.splits.data(), w.runs.data(), w.pieces.data(), 0, (int32_t)w.splits.size(), B, ins, del, split, chars, src, parts);
}

int main()
{
    std::mt19937      rng(2468);
    const int         moves[5][2] = {{0, 0}, {5, 0}, {0, 7}, {3, 4}, {255, 255}};
    uint8_t           chars[64], src[64];
    str_er_split_part parts[ld::MAX_NODES];

    // small alphabets inside the full one, every lattice of up to 2 runs of up to 3 atoms: the other characters cost 255 everywhere and the
    // live costs stay below 40, so that no path through a dead character can win
    for (int n = 2; n <= 3; ++n)
        for (int shape = 0; shape < 13; ++shape)
            for (const auto &mv : moves)
                for (int rep = 0; rep < 6; ++rep) {
                    std::vector<int> cuts;
                    if (shape >= 1 && shape < 4) cuts = {shape - 1};
                    if (shape >= 4) cuts = {(shape - 4) / 3, (shape - 4) % 3};
                    const int hi = rep % 2 ? 4 : 40, split = rep < 2 ? 0 : rep < 4 ? 8 : 255;
                    int       col = 0;
                    Word      w = make_word(cuts, [&] { const int a = col++ % 65; return (uint8_t)(a < n ? rng() % hi : 255); });
                    std::vector<uint8_t> B(wd::TABLE, 255);
                    for (int a = 0; a <= n; ++a)
                        for (int b = 0; b <= n; ++b) B[(a == n ? wd::E : a) * wd::STATES + (b == n ? wd::E : b)] = (uint8_t)(rng() % hi);
                    const str_er_lattice_decode r = decode(w, B.data(), mv[0], mv[1], split, chars, src, parts);
                    CHECK(r.cost == brute(w, 0, 0, wd::E, B.data(), n, mv[0], mv[1], split));
                    CHECK(r.cost == path_cost(w, B.data(), chars, src, r, parts, mv[0], mv[1], split));
                    CHECK(r.cost <= r.read_cost && r.n_sub + r.n_ins == r.n_chars && r.n_sub + r.n_del == r.n_parts && r.first_part == 0);
                    CHECK(r.n_parts >= (int)cuts.size() && r.n_parts <= w.nodes() && r.read_cost == wd::read_cost(w.runs.data(), (int)cuts.size(), B.data()));
                    CHECK((mv[0] > 0 || r.n_ins == 0) && (mv[1] > 0 || r.n_del == 0));
                    for (int k = 0; k < 64; ++k) CHECK(k < r.n_chars ? chars[k] < n : (chars[k] == 0xFF && src[k] == 0xFF));
                }

    // random words on the full alphabet: the path's cost is the cost, the identities hold, and without cuts the word decoder's bytes
    for (int it = 0; it < 200; ++it) {
        const int        R = (int)(rng() % 9);
        std::vector<int> cuts((size_t)R);
        for (auto &k : cuts) k = it % 4 ? (int)(rng() % 4) : 0;
        Word w = make_word(cuts, [&] { return (uint8_t)(rng() % 10 == 0 ? rng() % 24 : 60 + rng() % 196); });
        std::vector<uint8_t> B(wd::TABLE);
        for (auto &v : B) v = (uint8_t)(rng() % 256);
        const auto &mv = moves[it % 5];
        const int   split = it % 3 == 0 ? 0 : it % 3 == 1 ? 8 : 255;
        const str_er_lattice_decode r = decode(w, B.data(), mv[0], mv[1], split, chars, src, parts);
        CHECK(r.cost == path_cost(w, B.data(), chars, src, r, parts, mv[0], mv[1], split));
        CHECK(r.cost <= r.read_cost && r.n_sub + r.n_ins == r.n_chars && r.n_sub + r.n_del == r.n_parts && r.n_chars <= 2 * r.n_parts && r.n_parts >= R);
        uint8_t wc[64], ws[64];
        const str_er_word_decode d = wd::decode_word(w.runs.data(), R, B.data(), mv[0], mv[1], wc, ws);
        CHECK(r.cost <= d.cost && r.read_cost == d.read_cost);
        if (it % 4 == 0) {
            CHECK(r.cost == d.cost && r.n_chars == d.n_chars && r.n_sub == d.n_sub && r.n_del == d.n_del && r.n_ins == d.n_ins && r.n_parts == R);
            CHECK(!std::memcmp(chars, wc, 64) && !std::memcmp(src, ws, 64));
            for (int t = 0; t < R; ++t) CHECK(parts[t].run == t && parts[t].piece == -1);
        }
    }

    // hand-made words
    {
        std::vector<uint8_t> B(wd::TABLE, 0);
        B[wd::E * wd::STATES + wd::E] = 9;
        Word w = make_word({}, [] { return (uint8_t)0; });          // N = 0
        str_er_lattice_decode r = decode(w, B.data(), 64, 64, 8, chars, src, parts);
        CHECK(r.cost == 9 && r.read_cost == 9 && r.n_chars == 0 && r.n_parts == 0 && chars[0] == 0xFF && src[0] == 0xFF);

        w = make_word({0}, [] { return (uint8_t)7; });               // N = 1, all-equal rows: the smallest label, the whole run
        r = decode(w, B.data(), 64, 64, 8, chars, src, parts);
        CHECK(r.cost == 7 && r.n_chars == 1 && r.n_sub == 1 && r.n_parts == 1 && chars[0] == 0 && src[0] == 0 && parts[0].run == 0 && parts[0].piece == -1);

        // all-equal rows and table, three cuts, SPLIT = 0: every segmentation ties at one row a part, so fewer parts are cheaper and the
        // whole run wins; with the rows at 0 every path ties and the smaller i wins from the end backwards: the whole run again
        w = make_word({3}, [] { return (uint8_t)5; });
        r = decode(w, B.data(), 0, 0, 0, chars, src, parts);
        CHECK(r.cost == 5 && r.n_parts == 1 && parts[0].piece == -1 && r.n_chars == 1);
        w = make_word({3}, [] { return (uint8_t)0; });
        r = decode(w, B.data(), 0, 0, 0, chars, src, parts);
        CHECK(r.cost == 0 && r.n_parts == 1 && parts[0].piece == -1 && r.n_chars == 1 && chars[0] == 0);
        // ... and only the order of i decides between (0, 2) and (1, 2) into node 2 of a run of 2 atoms when piece (0, 1) is free too
        r = decode(make_word({1}, [] { return (uint8_t)0; }), B.data(), 0, 0, 0, chars, src, parts);
        CHECK(r.n_parts == 1 && parts[0].piece == -1);
        // SUB before DEL on a tie: two runs of 3s under a zero table with DEL = 3: reading the second costs what dropping it costs
        w = make_word({0, 0}, [] { return (uint8_t)3; });
        r = decode(w, B.data(), 0, 3, 8, chars, src, parts);
        CHECK(r.cost == 6 && r.n_sub == 2 && r.n_del == 0 && r.n_chars == 2 && src[0] == 0 && src[1] == 1);
        // ... and with DEL = 2 the first is dropped, the second read from the boundary (again a tie with dropping it behind a read one)
        r = decode(w, B.data(), 0, 2, 8, chars, src, parts);
        CHECK(r.cost == 5 && r.n_sub == 1 && r.n_del == 1 && r.n_chars == 1 && src[0] == 1 && r.n_parts == 2);

        // N = 32 in 8 runs of 4 atoms and in 32 uncut runs, N = 33: maximal values everywhere
        B.assign(wd::TABLE, 255);
        w = make_word(std::vector<int>(8, 3), [] { return (uint8_t)255; });
        r = decode(w, B.data(), 255, 255, 255, chars, src, parts);
        // (every run whole and dropped: 255 a run; a part more costs SPLIT and a drop of its own)
        CHECK(r.cost == 9 * 255 && r.read_cost == 17 * 255 && r.n_parts == 8 && r.n_del == 8 && r.n_chars == 0 && w.nodes() == 32);
        r = decode(w, B.data(), 0, 0, 255, chars, src, parts);
        CHECK(r.cost == 17 * 255 && r.n_parts == 8 && r.n_sub == 8 && r.n_chars == 8);
        w = make_word(std::vector<int>(32, 0), [] { return (uint8_t)255; });
        r = decode(w, B.data(), 255, 255, 255, chars, src, parts);
        CHECK(r.cost == 33 * 255 && r.read_cost == 65 * 255 && r.n_parts == 32 && r.n_del == 32 && r.n_chars == 0);
        std::vector<int> c33(8, 3);
        c33.push_back(0);
        w = make_word(c33, [] { return (uint8_t)255; });
        r = decode(w, B.data(), 255, 255, 255, chars, src, parts);
        CHECK(w.nodes() == 33 && r.cost == -1 && r.read_cost == 19 * 255 && r.n_chars == 0 && r.n_sub == 0 && r.n_del == 0 && r.n_ins == 0 && r.n_parts == 0);
        CHECK(chars[0] == 0xFF && src[63] == 0xFF);
        // a split that pays: the run reads dear, its two halves read cheap, and the table likes the pair
        w = make_word({1}, [] { return (uint8_t)200; });
        w.pieces[0 * 65 + 53] = 0; w.pieces[1 * 65 + 49] = 0;          // (0, 1) reads 'r', (1, 2) reads 'n'
        w.runs[48] = 40;                                               // the run reads 'm'
        B.assign(wd::TABLE, 30);
        r = decode(w, B.data(), 0, 0, 8, chars, src, parts);
        CHECK(r.cost == 30 + 0 + 30 + 0 + 8 + 30 && r.n_parts == 2 && r.n_chars == 2 && chars[0] == 53 && chars[1] == 49 && src[0] == 0 && src[1] == 1);
        CHECK(parts[0].run == 0 && parts[0].piece == 0 && parts[1].piece == 1);
        r = decode(w, B.data(), 0, 0, 255, chars, src, parts);
        CHECK(r.cost == 30 + 40 + 30 && r.n_parts == 1 && r.n_chars == 1 && chars[0] == 48 && parts[0].piece == -1);
    }

    CHECK(ld::params_ok(0, 0, 0) && ld::params_ok(255, 255, 255) && !ld::params_ok(0, 0, 256) && !ld::params_ok(0, 0, -1) && !ld::params_ok(256, 0, 8) &&
          !ld::params_ok(0, -1, 8));

    // the flag in a detect call: it rides on STR_ER_WANT_RUN_SPLIT, its refusals name it, a missing table is a state error, no lexicon and no
    // STR_ER_WANT_WORD_DECODE is needed
    {
        using namespace str_er_host;
        const uint32_t  grouped = STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP;
        const uint32_t  read = grouped | STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_WORDS | STR_ER_WANT_RUN_READ, spl = read | STR_ER_WANT_RUN_SPLIT;
        const uint32_t  lat = spl | STR_ER_WANT_LATTICE_DECODE;
        const CallShape frames{true, true, false, false}, planes{false, false, false, false}, strip{false, true, true, false};
        const auto      names = [](const StageVerdict &v) { return v.msg && std::strstr(v.msg, "STR_ER_WANT_LATTICE_DECODE") != nullptr; };
        CHECK(check_stages(lat, frames, true, true, false, true).code == STR_ER_OK && check_stages(lat, frames, true, true, false, true).msg == nullptr);
        StageVerdict v = check_stages(lat, frames, true, true, true, false);
        CHECK(v.code == STR_ER_ESTATE && names(v) && std::strstr(v.msg, "bigram"));
        v = check_stages(lat, frames, true, true, true);                        // (the five-argument call: no table)
        CHECK(v.code == STR_ER_ESTATE && names(v));
        v = check_stages(lat & ~STR_ER_WANT_RUN_SPLIT, frames, true, true, true, true);
        CHECK(v.code == STR_ER_EINVAL && names(v) && std::strstr(v.msg, "STR_ER_WANT_RUN_SPLIT"));
        v = check_stages(lat & ~STR_ER_WANT_RUN_SPLIT, frames, true, true, false, false);      // (the flag's own rule comes before the table's)
        CHECK(v.code == STR_ER_EINVAL && names(v));
        v = check_stages(lat & ~STR_ER_WANT_RUN_READ, frames, true, true, true, true);         // (ahead of _RUN_SPLIT's rule: the refusal names this flag)
        CHECK(v.code == STR_ER_EINVAL && names(v));
        v = check_stages(grouped | STR_ER_WANT_LATTICE_DECODE, frames, true, true, true, true);
        CHECK(v.code == STR_ER_EINVAL && names(v));
        v = check_stages(lat, planes, true, true, true, true);
        CHECK(v.code == STR_ER_EINVAL && names(v));
        v = check_stages(lat, strip, true, true, true, true);
        CHECK(v.code == STR_ER_EINVAL && names(v));
        v = check_stages(lat, frames, true, false, false, false);               // (no model either: the model's rule comes before the table's)
        CHECK(v.code == STR_ER_ESTATE && v.msg && std::strstr(v.msg, "STR_ER_WANT_RUN_READ"));
        v = check_stages(lat | STR_ER_WANT_WORD_MATCH, frames, true, true, false, true);       // (beside the matcher: it still needs its lexicon)
        CHECK(v.code == STR_ER_ESTATE && v.msg && std::strstr(v.msg, "STR_ER_WANT_WORD_MATCH"));
        CHECK(check_stages(lat | STR_ER_WANT_WORD_MATCH | STR_ER_WANT_WORD_DECODE, frames, true, true, true, true).code == STR_ER_OK);
        v = check_stages(lat | STR_ER_WANT_WORD_DECODE, frames, true, true, false, false);     // (both need the table: the decoder's rule is listed first)
        CHECK(v.code == STR_ER_ESTATE && v.msg && std::strstr(v.msg, "STR_ER_WANT_WORD_DECODE"));
        // without the flag nothing changes: the verdicts of the calls the other flags make, with and without a table
        for (const uint32_t st : {spl, spl | STR_ER_WANT_WORD_MATCH, spl | STR_ER_WANT_WORD_DECODE, read, grouped, (uint32_t)STR_ER_STAGE_ALL, spl & ~STR_ER_WANT_RUN_READ, 0u})
            for (const CallShape &k : {frames, planes, strip})
                for (int cs = 0; cs < 16; ++cs) {
                    const StageVerdict x = check_stages(st, k, cs & 1, cs & 2, cs & 4, cs & 8);
                    CHECK(!names(x));
                    if (!(st & STR_ER_WANT_WORD_DECODE)) {
                        const StageVerdict y = check_stages(st, k, cs & 1, cs & 2, cs & 4, !(cs & 8));
                        CHECK(x.code == y.code && x.msg == y.msg);
                    }
                }
        CHECK(STR_ER_WANT_LATTICE_DECODE == (1u << 26) && STR_ER_WANT_LATTICE_DECODE == 67108864u);
    }

    std::printf("%ld checks, %ld wrong\n", n_checks, n_wrong);
    return n_wrong ? 1 : 0;
}
