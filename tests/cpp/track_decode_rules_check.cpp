// track_decode_rules_check.cpp -- the rules of the track decode (csrc/track_decode_rules.h, the code the host entry point runs) on the
// CPU, under the host sanitizers: the cost of every neighbour from the prefix and suffix tables against the full recurrence on the
// edited string, the neighbour numbering at the lengths where DEL and INS switch off, the record of decode_track against its own
// properties on random tracks (members of 0 .. 33 rows, strings driven to 1 and 32 labels), the argument checks, and the rules of
// STR_ER_WANT_TRACK_DECODE in check_stages (csrc/stage_rules.h) with read_plan (csrc/read_plan.h).  A program of its own; prints
// "<checks> checks, <wrong> wrong".
#include "../../scene-text-recognition_amd/csrc/read_plan.h"
#include "../../scene-text-recognition_amd/csrc/stage_rules.h"
#include "../../scene-text-recognition_amd/csrc/track_decode_rules.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace td = str_er_td;
namespace wd = str_er_wd;

static long n_checks = 0, n_wrong = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++n_checks;                                                                  \
        if (!(cond)) { ++n_wrong; std::printf("line %d: %s\n", __LINE__, #cond); }   \
    } while (0)

static std::vector<uint8_t> random_rows(std::mt19937 &rng, int m, int lo, int hi)
{
    std::vector<uint8_t> C((size_t)std::max(m, 1) * 65);
    for (auto &v : C) v = (uint8_t)(lo + (int)(rng() % (unsigned)(hi - lo + 1)));
    return C;
}

// every neighbour of s from the tables against the recurrence on the edited string; returns how many neighbours exist
static int check_neighbours(const uint8_t *C, int m, const uint8_t *s, int l, int ins, int del)
{
    static td::Tables T;
    td::make_tables(C, m, s, l, ins, del, T);
    CHECK(T.F[l][m] == td::align_cost(C, m, s, l, ins, del));
    CHECK(T.G[0][0] == T.F[l][m]);
    int n = 0;
    for (int x = 0; x < td::N_NEIGHBOURS; ++x) {
        int j, a, g;
        if (!td::neighbour(x, l, j, a, g)) continue;
        ++n;
        uint8_t   t[td::MAX_LEN + 1];
        const int len = td::apply_neighbour(s, l, j, a, g, t);
        const int32_t want = td::align_cost(C, m, t, len, ins, del), got = td::joined_cost(T, C, m, j, a, g, ins);
        ++n_checks;
        if (want != got) { ++n_wrong; std::printf("neighbour %d of l = %d, m = %d: %d, the recurrence gives %d\n", x, l, m, got, want); }
    }
    return n;
}

int main()
{
    std::mt19937 rng(4242);

    // the neighbours from the tables, at every kind of length and row count
    const int lens[] = {1, 2, 3, 7, 31, 32}, ms[] = {0, 1, 2, 8, 9, 17, 32}, pairs[4][2] = {{64, 64}, {1, 255}, {255, 1}, {13, 40}};
    for (const int l : lens)
        for (const int m : ms)
            for (const auto &pr : pairs) {
                if ((l > 7 || m > 9) && &pr != &pairs[(l + m) % 4]) continue;          // (the large shapes with one pair each)
                const std::vector<uint8_t> C = random_rows(rng, m, 0, (l + m) % 2 ? 255 : 30);
                uint8_t                    s[td::MAX_LEN];
                for (int j = 0; j < l; ++j) s[j] = (uint8_t)(rng() % 65);
                const int n = check_neighbours(C.data(), m, s, l, pr[0], pr[1]);
                CHECK(n == l * 65 + (l > 1 ? l : 0) + (l < 32 ? (l + 1) * 65 : 0));
            }

    // the numbering
    {
        int j, a, g;
        CHECK(td::neighbour(0, 1, j, a, g) && j == 0 && a == 0 && g == 1);
        CHECK(td::neighbour(64, 1, j, a, g) && j == 0 && a == 64);
        CHECK(!td::neighbour(65, 1, j, a, g) && td::neighbour(65, 2, j, a, g) && j == 1 && a == 0 && g == 2);
        CHECK(!td::neighbour(2080, 1, j, a, g) && td::neighbour(2080, 2, j, a, g) && j == 0 && a == -1 && g == 1);
        CHECK(td::neighbour(2111, 32, j, a, g) && j == 31 && !td::neighbour(2111, 31, j, a, g));
        CHECK(td::neighbour(2112, 1, j, a, g) && j == 0 && a == 0 && g == 0);
        CHECK(td::neighbour(2112 + 65 + 3, 1, j, a, g) && j == 1 && a == 3 && g == 1 && !td::neighbour(2112 + 130, 1, j, a, g));
        CHECK(td::neighbour(4191, 31, j, a, g) && j == 31 && a == 64 && g == 31 && !td::neighbour(4192, 31, j, a, g));
        CHECK(!td::neighbour(2112, 32, j, a, g) && !td::neighbour(4256, 32, j, a, g));
        CHECK(td::params_ok(1, 1, 0) && td::params_ok(255, 255, 64) && !td::params_ok(0, 64, 8) && !td::params_ok(64, 256, 8) && !td::params_ok(64, 64, 65) &&
              !td::params_ok(64, 64, -1));
    }

    // whole tracks: the record against its own properties
    for (int trial = 0; trial < 40; ++trial) {
        const int            n_words = 1 + (int)(rng() % 6);
        std::vector<int32_t> first, n_of;
        std::vector<uint8_t> costs;
        const int            kinds[] = {0, 1, 2, 3, 5, 8, 31, 32, 33};
        for (int w = 0; w < n_words; ++w) {
            const int m = trial % 5 == 0 ? kinds[rng() % 9] : 1 + (int)(rng() % 5);
            first.push_back((int32_t)(costs.size() / 65)); n_of.push_back(m);
            const std::vector<uint8_t> C = random_rows(rng, m, 0, 255);
            if (m > 0) costs.insert(costs.end(), C.begin(), C.end());
        }
        if (costs.empty()) costs.resize(65);
        std::vector<uint8_t> B(wd::TABLE);
        const int            tables[] = {0, 255, 40, 90}, top = tables[trial % 4];
        for (auto &v : B) v = (uint8_t)(top == 0 ? 0 : top == 255 ? 255 : rng() % (unsigned)top);
        const int dec_ins = trial % 3 == 0 ? 1 : 0, dec_del = trial % 3 == 1 ? 64 : 0, ins = pairs[trial % 4][0], del = pairs[trial % 4][1], rounds = trial % 7 == 0 ? 0 : trial % 7 == 1 ? 1 : 64;
        std::vector<str_er_word_decode> dec((size_t)n_words);
        std::vector<uint8_t>            dchars((size_t)n_words * 64), dsrc(64);
        for (int w = 0; w < n_words; ++w)
            dec[(size_t)w] = wd::decode_word(costs.data() + (size_t)first[(size_t)w] * 65, n_of[(size_t)w], B.data(), dec_ins, dec_del, dchars.data() + (size_t)w * 64, dsrc.data());
        std::vector<int32_t> members;
        const int            count = (int)(rng() % 7);
        for (int i = 0; i < count; ++i) members.push_back((int32_t)(rng() % (unsigned)n_words));
        uint8_t              chars[32];
        std::vector<int32_t> own((size_t)std::max(count, 1), 7);
        const str_er_track_decode r = td::decode_track(costs.data(), first.data(), n_of.data(), members.data(), count, dec.data(), dchars.data(), B.data(), ins, del, rounds,
                                                       chars, own.data());
        int n_used = 0, n_seeds = 0;
        for (const int32_t w : members) {
            n_used += n_of[(size_t)w] <= 32;
            n_seeds += n_of[(size_t)w] <= 32 && dec[(size_t)w].n_chars >= 1 && dec[(size_t)w].n_chars <= 32;
        }
        CHECK(r.n_used == n_used);
        if (n_seeds == 0) {
            CHECK(r.cost == -1 && r.seed_cost == -1 && r.lm_cost == -1 && r.n_chars == 0 && r.n_edits == 0 && r.converged == 0 && r.seed_member == -1);
            for (int i = 0; i < count; ++i) CHECK(own[(size_t)i] == -1);
            for (const uint8_t c : chars) CHECK(c == 0xFF);
            continue;
        }
        CHECK(r.n_chars >= 1 && r.n_chars <= 32 && r.n_edits <= rounds && (rounds > 0 || r.converged == 0));
        int32_t sum = td::lm_cost(chars, r.n_chars, B.data());
        CHECK(sum == r.lm_cost);
        for (int i = 0; i < count; ++i) {
            const int32_t w = members[(size_t)i];
            if (n_of[(size_t)w] > 32) { CHECK(own[(size_t)i] == -1); continue; }
            CHECK(own[(size_t)i] == td::align_cost(costs.data() + (size_t)first[(size_t)w] * 65, n_of[(size_t)w], chars, r.n_chars, ins, del));
            sum += own[(size_t)i];
        }
        CHECK(sum == r.cost && r.cost >= 0 && r.cost <= r.seed_cost);
        for (int k = r.n_chars; k < 32; ++k) CHECK(chars[k] == 0xFF);
        if (r.converged) {          // no neighbour below cost, by the recurrence
            for (int x = 0; x < td::N_NEIGHBOURS; x += 1 + (int)(rng() % 5)) {
                int j, a, g;
                if (!td::neighbour(x, r.n_chars, j, a, g)) continue;
                uint8_t   t[td::MAX_LEN + 1];
                const int len = td::apply_neighbour(chars, r.n_chars, j, a, g, t);
                int32_t   J = td::lm_cost(t, len, B.data());
                for (const int32_t w : members)
                    if (n_of[(size_t)w] <= 32) J += td::align_cost(costs.data() + (size_t)first[(size_t)w] * 65, n_of[(size_t)w], t, len, ins, del);
                CHECK(J >= r.cost);
            }
        }
    }

    // the tracks' checks
    {
        const int32_t tf[2] = {0, 2}, tc[2] = {2, 1}, mem[3] = {0, 1, 1}, big[1] = {1025}, ok[1] = {1024};
        std::vector<int32_t> many(1025, 0);
        CHECK(td::tracks_check(tf, tc, mem, 3, 2, 2) == STR_ER_OK);
        CHECK(td::tracks_check(tf, tc, mem, 3, 2, 1) == STR_ER_EINVAL);
        CHECK(td::tracks_check(tf, tc, mem, 2, 2, 2) == STR_ER_EINVAL);
        CHECK(td::tracks_check(tf, big, many.data(), 1025, 1, 1) == STR_ER_ECAPACITY);
        CHECK(td::tracks_check(tf, ok, many.data(), 1025, 1, 1) == STR_ER_OK);
    }

    // the flag's rules: refused on the strip path, on the per-plane calls, without _LINE_LINKS, without _WORD_DECODE (and so without
    // _RUN_READ); accepted without _WORD_MATCH and without a lexicon; ESTATE without a table; a call without the flag as before
    {
        using str_er_host::CallShape;
        using str_er_host::check_stages;
        const uint32_t  base = STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_LINKS | STR_ER_WANT_LINE_WORDS |
                              STR_ER_WANT_RUN_READ | STR_ER_WANT_WORD_DECODE;
        const uint32_t  full = base | STR_ER_WANT_TRACK_DECODE;
        const CallShape frames{true, true, false, false}, strip{false, false, true, false}, planes{false, false, false, false};
        const auto      names = [](const str_er_host::StageVerdict &v) { return v.msg && std::strstr(v.msg, "STR_ER_WANT_TRACK_DECODE") != nullptr; };
        CHECK(check_stages(full, frames, true, true, false, true).code == STR_ER_OK);
        CHECK(check_stages(full, frames, true, true, false, false).code == STR_ER_ESTATE);
        CHECK(check_stages(full, strip, true, true, false, true).code == STR_ER_EINVAL && names(check_stages(full, strip, true, true, false, true)));
        CHECK(check_stages(full, planes, true, true, false, true).code == STR_ER_EINVAL && names(check_stages(full, planes, true, true, false, true)));
        for (const uint32_t drop : {STR_ER_WANT_LINE_LINKS, STR_ER_WANT_WORD_DECODE, STR_ER_WANT_RUN_READ}) {
            const auto v = check_stages(full & ~drop, frames, true, true, false, true);
            CHECK(v.code == STR_ER_EINVAL && names(v));
        }
        for (uint32_t bits = 0; bits < 4096; ++bits) {          // without the flag: no verdict names it
            const uint32_t st = STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | (bits << 17);
            for (const CallShape &k : {frames, strip, planes}) CHECK(!names(check_stages(st, k, true, true, bits & 1, bits & 2)));
        }
        // the plan: the track decode only with decode, on the decoder's set; every other field as without it
        for (int bits = 0; bits < 256; ++bits) {
            const bool m = bits & 1, d = bits & 2, s = bits & 4, la = bits & 8, t = bits & 16, f = bits & 32, lm = bits & 64, lt = bits & 128;
            str_er_host::ReadPlan p = str_er_host::read_plan(m, d, s, la, t, f, lm, lt, true), q = str_er_host::read_plan(m, d, s, la, t, f, lm, lt);
            CHECK(p.tdecode == d && !q.tdecode && (!p.tdecode || p.decode_set != str_er_host::SET_NONE));
            CHECK(p.match == q.match && p.decode == q.decode && p.split == q.split && p.lattice == q.lattice && p.track == q.track && p.lmatch == q.lmatch &&
                  p.ltrack == q.ltrack && p.rows[0] == q.rows[0] && p.rows[1] == q.rows[1] && p.fold_a == q.fold_a && p.parts[0] == q.parts[0] &&
                  p.parts[1] == q.parts[1] && p.match_set == q.match_set && p.decode_set == q.decode_set && p.lattice_set == q.lattice_set &&
                  p.lattice_match_set == q.lattice_match_set && p.lattice_track_set == q.lattice_track_set && p.result_set == q.result_set &&
                  p.split_down == q.split_down && p.run_probs == q.run_probs);
        }
    }

    std::printf("%ld checks, %ld wrong\n", n_checks, n_wrong);
    return n_wrong == 0 ? 0 : 1;
}
