// word_match_rules_check.cpp -- the rules of the lexicon matcher (csrc/word_match_rules.h, the code the host entry points run) on the CPU,
// under the host sanitizers: cost() at every threshold and next to it, the cost row of a run, the edit distance on cases computed by
// hand and against a plain recursion, the best / second merge, the band and the lexicon checks, and the rules of
// STR_ER_WANT_WORD_MATCH in check_stages (csrc/stage_rules.h).  A program of its own; prints "<checks> checks, <wrong> wrong".
#include "../../scene-text-recognition_amd/csrc/stage_rules.h"
#include "../../scene-text-recognition_amd/csrc/word_match_rules.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

namespace wm = str_er_wm;

static long n_checks = 0, n_wrong = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++n_checks;                                                                  \
        if (!(cond)) { ++n_wrong; std::printf("line %d: %s\n", __LINE__, #cond); }   \
    } while (0)

// D[i][j] by the recurrence as the contract writes it, by recursion
static int32_t rec(const uint8_t *C, const uint8_t *e, int i, int j, int ins, int del)
{
    if (i == 0) return j * ins;
    if (j == 0) return i * del;
    const int32_t a = rec(C, e, i - 1, j - 1, ins, del) + C[(i - 1) * 65 + e[j - 1]], b = rec(C, e, i - 1, j, ins, del) + del,
                  c = rec(C, e, i, j - 1, ins, del) + ins;
    return std::min(a, std::min(b, c));
}

static std::vector<uint8_t> rows(int m, int fill) { return std::vector<uint8_t>((size_t)m * 65, (uint8_t)fill); }

int main()
{
    double T[255];
    wm::thresholds(T);
    // the table: the eight literals scaled by powers of two, falling
    CHECK(T[0] == 1.0 && T[8] == 0.5 && T[16] == 0.25 && T[4] == 0x1.6a09e667f3bcdp-1 && T[12] == 0x1.6a09e667f3bcdp-2);
    for (int c = 0; c < 255; ++c) {
        CHECK(T[c] == std::ldexp(wm::MANTISSA[c % 8], -(c / 8)));
        if (c) CHECK(T[c] < T[c - 1]);
        // at the threshold, and one step below and above it
        CHECK(wm::cost(T[c], T) == c);
        CHECK(wm::cost(std::nextafter(T[c], 0.0), T) == (c < 254 ? c + 1 : 255));
        CHECK(wm::cost(std::nextafter(T[c], 2.0), T) == c);
    }
    CHECK(wm::cost(0.0, T) == 255 && wm::cost(-0.0, T) == 255 && wm::cost(1.0, T) == 0 && wm::cost(2.0, T) == 0);
    CHECK(wm::cost(std::numeric_limits<double>::quiet_NaN(), T) == 255 && wm::cost(-1.0, T) == 255);
    CHECK(wm::cost(std::numeric_limits<double>::infinity(), T) == 0 && wm::cost(-std::numeric_limits<double>::infinity(), T) == 255);
    CHECK(wm::cost(std::numeric_limits<double>::denorm_min(), T) == 255 && wm::cost(0.5, T) == 8 && wm::cost(0.75, T) == 4);

    // the alphabet and the case pairs
    {
        const char *table = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz&()";
        int         known = 0;
        for (int b = 0; b < 256; ++b) {
            const char *at = b ? std::strchr(table, b) : nullptr;
            CHECK(wm::char_label((unsigned char)b) == (at ? (int)(at - table) : -1));
            known += at != nullptr;
        }
        CHECK(known == 65);
        for (int a = 0; a < 65; ++a) {
            const int p = wm::fold_partner(a);
            CHECK(wm::fold_partner(p) == a);
            CHECK((p == a) == !((table[a] >= 'A' && table[a] <= 'Z') || (table[a] >= 'a' && table[a] <= 'z')));
            if (p != a) CHECK((table[a] ^ table[p]) == 0x20);
        }
    }

    // the cost row of a run: permuted labels, labels outside the alphabet, a missing character, a label named twice, fold-case
    {
        const int32_t labels[6] = {36, 10, 99, -1, 0, 10};            // 'a', 'A', outside, outside, '0', 'A' again
        const double  prob[6] = {0.5, 0.25, 1.0, 1.0, T[100], 1.0};
        uint8_t       C[65];
        wm::cost_row(prob, 6, labels, false, T, C);
        CHECK(C[36] == 8 && C[10] == 16 && C[0] == 100 && C[1] == 255 && C[64] == 255 && C[11] == 255);
        wm::cost_row(prob, 6, labels, true, T, C);
        CHECK(C[36] == 8 && C[10] == 8 && C[0] == 100 && C[11] == 255 && C[37] == 255);
        wm::cost_row(prob, 0, labels, true, T, C);
        for (int a = 0; a < 65; ++a) CHECK(C[a] == 255);
    }

    // the edit distance, by hand (INS = DEL = 64)
    const uint8_t AB[2] = {10, 11}, A[1] = {10}, a_low[1] = {36};
    {   // three runs for AB with a noise run in the middle: A, DEL, B
        std::vector<uint8_t> C = rows(3, 200);
        C[0 * 65 + 10] = 0; C[2 * 65 + 11] = 0;
        CHECK(wm::entry_cost(C.data(), 3, AB, 2, 64, 64, false) == 64);
        CHECK(wm::entry_cost(C.data(), 3, AB, 2, 64, 255, false) == 255);          // (three runs for two characters: every path has a DEL)
    }
    {   // one run for AB: the run is A and B has no run of its own (8 + 64), not the other way round (64 + 16)
        std::vector<uint8_t> C = rows(1, 255);
        C[10] = 8; C[11] = 16;
        CHECK(wm::entry_cost(C.data(), 1, AB, 2, 64, 64, false) == 72);
        C[10] = 30;
        CHECK(wm::entry_cost(C.data(), 1, AB, 2, 64, 64, false) == 80);
        CHECK(wm::entry_cost(C.data(), 1, AB, 2, 1, 64, false) == 17);
    }
    {   // no runs; two runs for A
        CHECK(wm::entry_cost(nullptr, 0, AB, 2, 64, 7, false) == 128 && wm::entry_cost(nullptr, 0, A, 1, 3, 7, false) == 3);
        std::vector<uint8_t> C = rows(2, 255);
        C[0 * 65 + 10] = 10; C[1 * 65 + 10] = 3;
        CHECK(wm::entry_cost(C.data(), 2, A, 1, 64, 64, false) == 67);
        CHECK(wm::entry_cost(C.data(), 2, A, 1, 64, 5, false) == 8);
    }
    {   // the extremes at m = l = 32
        uint8_t e[32];
        for (int j = 0; j < 32; ++j) e[j] = (uint8_t)(j * 2);
        std::vector<uint8_t> C = rows(32, 255);
        CHECK(wm::entry_cost(C.data(), 32, e, 32, 255, 255, false) == 32 * 255);
        CHECK(wm::entry_cost(C.data(), 32, e, 1, 255, 255, false) == 32 * 255);      // (one substitution, 31 DEL)
        C = rows(32, 0);
        CHECK(wm::entry_cost(C.data(), 32, e, 32, 255, 255, false) == 0);
        CHECK(wm::entry_cost(C.data(), 32, e, 30, 1, 2, false) == 4);
    }
    {   // fold-case
        std::vector<uint8_t> C = rows(1, 255);
        C[10] = 5; C[36] = 100;
        CHECK(wm::entry_cost(C.data(), 1, a_low, 1, 64, 64, false) == 100 && wm::entry_cost(C.data(), 1, a_low, 1, 64, 64, true) == 5);
        CHECK(wm::entry_cost(C.data(), 1, A, 1, 64, 64, true) == 5);
    }
    // ... and against the recursion, on small random cases
    {
        std::mt19937 rng(7);
        for (int t = 0; t < 400; ++t) {
            const int m = (int)(rng() % 6), l = 1 + (int)(rng() % 5), ins = 1 + (int)(rng() % 255), del = 1 + (int)(rng() % 255);
            std::vector<uint8_t> C((size_t)std::max(m, 1) * 65);
            for (uint8_t &v : C) v = (uint8_t)(rng() % 3 ? rng() % 256 : rng() % 8);
            uint8_t e[5];
            for (int j = 0; j < l; ++j) e[j] = (uint8_t)(rng() % 65);
            CHECK(wm::entry_cost(C.data(), m, e, l, ins, del, false) == rec(C.data(), e, m, l, ins, del));
        }
    }

    // the band
    CHECK(wm::in_band(5, 7, 2) && wm::in_band(5, 3, 2) && !wm::in_band(5, 8, 2) && !wm::in_band(5, 2, 2) && wm::in_band(5, 5, 0) && !wm::in_band(5, 6, 0));
    CHECK(wm::in_band(1, 32, 31) && wm::in_band(32, 1, 31) && wm::in_band(32, 32, 0) && !wm::in_band(33, 32, 31) && !wm::in_band(33, 33, 0));
    CHECK(wm::in_band(0, 2, 2) && !wm::in_band(0, 3, 2));
    CHECK(wm::params_ok(1, 1, 0) && wm::params_ok(255, 255, 31) && !wm::params_ok(0, 1, 0) && !wm::params_ok(1, 256, 0) && !wm::params_ok(1, 1, 32) &&
          !wm::params_ok(1, 1, -1));

    // best and second
    {
        wm::Best2 b;
        CHECK(wm::make_match(b, 9, 0).entry == -1 && wm::make_match(b, 9, 0).cost == -1 && wm::make_match(b, 9, 0).second_entry == -1 &&
              wm::make_match(b, 9, 0).second_cost == -1 && wm::make_match(b, 9, 0).free_cost == 9);
        b.add(wm::make_key(70, 5));
        CHECK(wm::make_match(b, 0, 1).entry == 5 && wm::make_match(b, 0, 1).cost == 70 && wm::make_match(b, 0, 1).second_entry == -1);
        b.add(wm::make_key(70, 3));              // a tie: the lower index wins, the other is second with the same cost
        b.add(wm::make_key(90, 0));
        str_er_word_match r = wm::make_match(b, 0, 3);
        CHECK(r.entry == 3 && r.cost == 70 && r.second_entry == 5 && r.second_cost == 70 && r.n_tried == 3);
        wm::Best2 o, e;
        o.add(wm::make_key(10, 9)); o.add(wm::make_key(80, 1));
        b.merge(o); b.merge(e);
        r = wm::make_match(b, 0, 5);
        CHECK(r.entry == 9 && r.cost == 10 && r.second_entry == 3 && r.second_cost == 70);
        CHECK(wm::make_key(0, 1 << 20) > wm::make_key(0, 5) && wm::make_key(1, 0) > wm::make_key(0, 1 << 20) && wm::make_key(16320, 1 << 20) != wm::NO_KEY);
    }

    // a word against a lexicon: AB, ab, ABC, B; two runs that read A and B
    {
        const char    bytes[] = "ABabABCB";
        const int32_t off[5] = {0, 2, 4, 7, 8};
        uint8_t       lab[8];
        for (int i = 0; i < 8; ++i) lab[i] = (uint8_t)wm::char_label((unsigned char)bytes[i]);
        std::vector<uint8_t> C = rows(2, 250);
        C[0 * 65 + 10] = 1; C[1 * 65 + 11] = 2; C[1 * 65 + 40] = 0;
        wm::MatchParams p;
        str_er_word_match r = wm::match_word(C.data(), 2, lab, off, 4, p, false);
        CHECK(r.entry == 0 && r.cost == 3 && r.second_entry == 3 && r.second_cost == 64 + 2 && r.free_cost == 1 && r.n_tried == 4);
        r = wm::match_word(C.data(), 2, lab, off, 4, p, true);
        CHECK(r.entry == 0 && r.cost == 3 && r.second_entry == 1 && r.second_cost == 3 && r.n_tried == 4);
        p.band = 0;
        r = wm::match_word(C.data(), 2, lab, off, 4, p, false);          // (ab without fold-case: two DEL and two INS beat two substitutions at 250)
        CHECK(r.entry == 0 && r.second_entry == 1 && r.second_cost == 256 && r.n_tried == 2);
        r = wm::match_word(C.data(), 2, lab, off, 0, p, false);
        CHECK(r.entry == -1 && r.cost == -1 && r.n_tried == 0 && r.free_cost == 1);
        std::vector<uint8_t> big = rows(33, 4);
        p.band = 31;
        r = wm::match_word(big.data(), 33, lab, off, 4, p, false);
        CHECK(r.entry == -1 && r.n_tried == 0 && r.free_cost == 33 * 4);
    }

    // what a lexicon may be
    {
        const char    ok[] = "AB&(", bad[] = "A B", long33[] = "012345678901234567890123456789012";
        const int32_t o2[3] = {0, 2, 4}, gap[3] = {1, 2, 4}, back[3] = {0, 2, 2}, o33[2] = {0, 33}, o32[2] = {0, 32}, o3[2] = {0, 3};
        const char   *why = nullptr;
        CHECK(wm::lexicon_check(ok, o2, 2, 0, &why) == STR_ER_OK && wm::lexicon_check(ok, o2, 2, STR_ER_LEXICON_FOLD_CASE, &why) == STR_ER_OK);
        CHECK(wm::lexicon_check(nullptr, nullptr, 0, 0, &why) == STR_ER_OK && wm::lexicon_check(long33, o32, 1, 0, &why) == STR_ER_OK);
        CHECK(wm::lexicon_check(ok, o2, 2, 2, &why) == STR_ER_EINVAL && wm::lexicon_check(ok, o2, -1, 0, &why) == STR_ER_EINVAL);
        CHECK(wm::lexicon_check(ok, gap, 2, 0, &why) == STR_ER_EINVAL && wm::lexicon_check(ok, back, 2, 0, &why) == STR_ER_EINVAL);
        CHECK(wm::lexicon_check(long33, o33, 1, 0, &why) == STR_ER_EINVAL && wm::lexicon_check(bad, o3, 1, 0, &why) == STR_ER_EINVAL && why != nullptr);
        CHECK(wm::lexicon_check(ok, o2, (1 << 20) + 1, 0, &why) == STR_ER_ECAPACITY && wm::lexicon_check(nullptr, o2, 2, 0, nullptr) == STR_ER_EINVAL);
    }

    // the flag in a detect call: it rides on STR_ER_WANT_RUN_READ, its refusals name it and come first, a missing lexicon is a state error
    {
        using namespace str_er_host;
        const uint32_t  grouped = STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP;
        const uint32_t  read = grouped | STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_WORDS | STR_ER_WANT_RUN_READ, match = read | STR_ER_WANT_WORD_MATCH;
        const CallShape frames{true, true, false, false}, planes{false, false, false, false}, strip{false, true, true, false};
        const auto      names = [](const StageVerdict &v) { return v.msg && std::strstr(v.msg, "STR_ER_WANT_WORD_MATCH") != nullptr; };
        CHECK(check_stages(match, frames, true, true, true).code == STR_ER_OK && check_stages(match, frames, true, true, true).msg == nullptr);
        StageVerdict v = check_stages(match, frames, true, true, false);
        CHECK(v.code == STR_ER_ESTATE && names(v) && std::strstr(v.msg, "lexicon"));
        v = check_stages(match, frames, true, true);                          // (the four-argument call: no lexicon)
        CHECK(v.code == STR_ER_ESTATE && names(v));
        v = check_stages(match & ~STR_ER_WANT_RUN_READ, frames, true, true, true);
        CHECK(v.code == STR_ER_EINVAL && names(v));
        v = check_stages(grouped | STR_ER_WANT_WORD_MATCH, frames, true, true, true);
        CHECK(v.code == STR_ER_EINVAL && names(v));
        v = check_stages(match, planes, true, true, true);
        CHECK(v.code == STR_ER_EINVAL && names(v));
        v = check_stages(match, strip, true, true, true);
        CHECK(v.code == STR_ER_EINVAL && names(v));
        v = check_stages(match, frames, true, false, false);                  // (no model either: the model's rule comes before the lexicon's)
        CHECK(v.code == STR_ER_ESTATE && v.msg && std::strstr(v.msg, "STR_ER_WANT_RUN_READ"));
        v = check_stages(match, frames, false, true, true);
        CHECK(v.code == STR_ER_ESTATE && !names(v));
        // without the flag the lexicon changes no verdict
        for (const uint32_t st : {read, grouped, (uint32_t)STR_ER_STAGE_ALL, read & ~STR_ER_WANT_LINE_WORDS, 0u})
            for (const CallShape &k : {frames, planes, strip})
                for (int cs = 0; cs < 4; ++cs) {
                    const StageVerdict x = check_stages(st, k, cs & 1, cs & 2, false), y = check_stages(st, k, cs & 1, cs & 2, true);
                    CHECK(x.code == y.code && x.msg == y.msg);
                }
        CHECK(STR_ER_WANT_WORD_MATCH == (1u << 22));
    }

    std::printf("%ld checks, %ld wrong\n", n_checks, n_wrong);
    return n_wrong ? 1 : 0;
}
