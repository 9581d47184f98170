// word_decode_rules_check.cpp -- the rules of the word decoder (csrc/word_decode_rules.h, the code the host entry points run) on the CPU,
// under the host sanitizers: the recurrence against an enumeration of every path on tables whose live part is 2 or 3 characters, the cost
// of the returned string recomputed from its labels and sources, the fixed vectors of the contract, read_cost, the table builder, and
// the rules of STR_ER_WANT_WORD_DECODE in check_stages (csrc/stage_rules.h).  A program of its own; prints "<checks> checks, <wrong> wrong".
#include "../../scene-text-recognition_amd/csrc/stage_rules.h"
#include "../../scene-text-recognition_amd/csrc/word_decode_rules.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace wd = str_er_wd;

static long n_checks = 0, n_wrong = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++n_checks;                                                                  \
        if (!(cond)) { ++n_wrong; std::printf("line %d: %s\n", __LINE__, #cond); }   \
    } while (0)

static int B_at(const uint8_t *B, int a, int b) { return B[a * wd::STATES + b]; }

// the cheapest path over the live characters 0 .. n - 1 by brute force: per run a drop or a reading, and behind either one inserted
// character that follows some character (prev: the last character, E for none)
static int32_t brute(const uint8_t *C, int m, int i, int prev, const uint8_t *B, int n, int ins, int del)
{
    if (i == m) return B_at(B, prev, wd::E);
    int32_t best = 1 << 30;
    const auto tail = [&](int32_t sofar, int p) {
        best = std::min(best, sofar + brute(C, m, i + 1, p, B, n, ins, del));
        if (ins > 0 && p != wd::E)
            for (int c = 0; c < n; ++c) best = std::min(best, sofar + B_at(B, p, c) + ins + brute(C, m, i + 1, c, B, n, ins, del));
    };
    if (del > 0) tail(del, prev);
    for (int b = 0; b < n; ++b) tail(B_at(B, prev, b) + C[i * 65 + b], b);
    return best;
}

// the cost of a returned string under the definition
static int32_t path_cost(const uint8_t *C, int m, const uint8_t *B, const uint8_t *chars, const uint8_t *src, int n_chars, int ins, int del)
{
    int     prev = wd::E, used = 0;
    int32_t s = 0;
    for (int k = 0; k < n_chars; ++k) {
        s += B_at(B, prev, chars[k]);
        if (src[k] & 0x80) s += ins;
        else { s += C[(src[k] & 0x7F) * 65 + chars[k]]; ++used; }
        prev = chars[k];
    }
    return s + B_at(B, prev, wd::E) + del * (m - used);
}

int main()
{
    std::mt19937 rng(12345);
    const int    pairs[6][2] = {{0, 0}, {5, 0}, {0, 7}, {3, 4}, {1, 1}, {255, 255}};
    uint8_t      chars[64], src[64];

    // small alphabets inside the full one: the other characters cost 255 everywhere and the live costs stay below 40, so that no path
    // through a dead character can win (a dead step costs 255 or more; a whole live path at most 3 * (39 + 39 + 39 + 39) + 39)
    for (int n = 2; n <= 3; ++n)
        for (int m = 0; m <= 3; ++m)
            for (const auto &pr : pairs)
                for (int rep = 0; rep < 30; ++rep) {
                    const int            hi = rep % 2 ? 4 : 40;
                    std::vector<uint8_t> C((size_t)std::max(m, 1) * 65, 255), B(wd::TABLE, 255);
                    for (int i = 0; i < m; ++i)
                        for (int a = 0; a < n; ++a) C[i * 65 + a] = (uint8_t)(rng() % hi);
                    for (int a = 0; a <= n; ++a)
                        for (int b = 0; b <= n; ++b) B[(a == n ? wd::E : a) * wd::STATES + (b == n ? wd::E : b)] = (uint8_t)(rng() % hi);
                    const int ins = pr[0] == 255 ? 255 : pr[0], del = pr[1];
                    const str_er_word_decode r = wd::decode_word(C.data(), m, B.data(), ins, del, chars, src);
                    CHECK(r.cost == brute(C.data(), m, 0, wd::E, B.data(), n, ins, del));
                    CHECK(r.cost == path_cost(C.data(), m, B.data(), chars, src, r.n_chars, ins, del));
                    CHECK(r.cost <= r.read_cost && r.n_sub + r.n_ins == r.n_chars && r.n_sub + r.n_del == m && r.read_cost == wd::read_cost(C.data(), m, B.data()));
                    CHECK((ins > 0 || r.n_ins == 0) && (del > 0 || r.n_del == 0));
                    for (int k = 0; k < 64; ++k) CHECK(k < r.n_chars ? chars[k] < n : (chars[k] == 0xFF && src[k] == 0xFF));
                }

    // random words on the full alphabet: the string's cost is the cost, the identities hold
    for (int it = 0; it < 200; ++it) {
        const int            m = (int)(rng() % 33);
        std::vector<uint8_t> C((size_t)std::max(m, 1) * 65), B(wd::TABLE);
        for (auto &v : C) v = (uint8_t)(rng() % 10 == 0 ? rng() % 24 : 60 + rng() % 196);
        for (auto &v : B) v = (uint8_t)(rng() % 256);
        const auto &pr = pairs[it % 6];
        const str_er_word_decode r = wd::decode_word(C.data(), m, B.data(), pr[0], pr[1], chars, src);
        CHECK(r.cost == path_cost(C.data(), m, B.data(), chars, src, r.n_chars, pr[0], pr[1]));
        CHECK(r.cost <= r.read_cost && r.n_sub + r.n_ins == r.n_chars && r.n_sub + r.n_del == m && r.n_chars <= 2 * m);
        if (m == 0) CHECK(r.cost == B[wd::E * wd::STATES + wd::E] && r.read_cost == r.cost && r.n_chars == 0);
    }

    // the fixed vectors
    {
        std::vector<uint8_t> C(5 * 65, 0), B(wd::TABLE, 0);
        str_er_word_decode   r = wd::decode_word(C.data(), 5, B.data(), 64, 64, chars, src);
        CHECK(r.cost == 0 && r.read_cost == 0 && r.n_chars == 5 && r.n_sub == 5 && r.n_del == 0 && r.n_ins == 0);
        for (int k = 0; k < 5; ++k) CHECK(chars[k] == 0 && src[k] == k);
        CHECK(chars[5] == 0xFF && src[5] == 0xFF);

        C.assign(32 * 65, 255); B.assign(wd::TABLE, 255);
        for (int i = 0; i < 32; ++i) C[i * 65 + 63] = 0;
        B[65 * 66 + 63] = B[63 * 66 + 64] = B[64 * 66 + 63] = B[64 * 66 + 65] = 0;
        r = wd::decode_word(C.data(), 32, B.data(), 1, 0, chars, src);
        CHECK(r.cost == 32 && r.n_chars == 64 && r.n_sub == 32 && r.n_ins == 32 && r.n_del == 0);
        for (int k = 0; k < 64; ++k) CHECK(chars[k] == (k % 2 ? 64 : 63) && src[k] == (k % 2 ? (0x80 | k / 2) : k / 2));
        CHECK(src[63] == 0x9F);

        C.assign(33 * 65, 255); B.assign(wd::TABLE, 255);
        r = wd::decode_word(C.data(), 32, B.data(), 255, 255, chars, src);
        CHECK(r.cost == 33 * 255 && r.read_cost == 65 * 255 && r.n_chars == 0 && r.n_del == 32 && r.n_sub == 0 && r.n_ins == 0 && chars[0] == 0xFF);
        r = wd::decode_word(C.data(), 33, B.data(), 255, 255, chars, src);
        CHECK(r.cost == -1 && r.read_cost == 67 * 255 && r.n_chars == 0 && r.n_sub == 0 && r.n_del == 0 && r.n_ins == 0 && chars[0] == 0xFF && src[63] == 0xFF);
    }

    // the parameters and the table builder
    {
        CHECK(wd::params_ok(0, 0) && wd::params_ok(255, 255) && !wd::params_ok(-1, 0) && !wd::params_ok(0, 256) && !wd::params_ok(256, 0));
        std::vector<double> tp(65 * 65, 0.5), st(65, 0.25), en(65, 1.0);
        tp[3 * 65 + 4] = 1.0; tp[0] = 0.0; tp[1] = -1.0;
        st[7] = 0.0;
        uint8_t out[wd::TABLE];
        wd::table_from_probs(tp.data(), st.data(), en.data(), out);
        CHECK(out[3 * 66 + 4] == 0 && out[0] == 255 && out[1] == 255 && out[2] == 8 && out[64 * 66 + 64] == 8);
        CHECK(out[65 * 66 + 0] == 16 && out[65 * 66 + 7] == 255 && out[0 * 66 + 65] == 0 && out[64 * 66 + 65] == 0 && out[65 * 66 + 65] == 0);
        wd::table_from_probs(tp.data(), nullptr, nullptr, out);
        for (int a = 0; a < 66; ++a) CHECK(out[a * 66 + 65] == 0 && out[65 * 66 + a] == 0);
        CHECK(out[5 * 66 + 6] == 8);
    }

    // the flag in a detect call: it rides on STR_ER_WANT_RUN_READ, its refusals name it, a missing table is a state error, no lexicon is needed
    {
        using namespace str_er_host;
        const uint32_t  grouped = STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP;
        const uint32_t  read = grouped | STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_WORDS | STR_ER_WANT_RUN_READ, dec = read | STR_ER_WANT_WORD_DECODE;
        const CallShape frames{true, true, false, false}, planes{false, false, false, false}, strip{false, true, true, false};
        const auto      names = [](const StageVerdict &v) { return v.msg && std::strstr(v.msg, "STR_ER_WANT_WORD_DECODE") != nullptr; };
        CHECK(check_stages(dec, frames, true, true, false, true).code == STR_ER_OK && check_stages(dec, frames, true, true, false, true).msg == nullptr);
        StageVerdict v = check_stages(dec, frames, true, true, true, false);
        CHECK(v.code == STR_ER_ESTATE && names(v) && std::strstr(v.msg, "bigram"));
        v = check_stages(dec, frames, true, true, true);                        // (the five-argument call: no table)
        CHECK(v.code == STR_ER_ESTATE && names(v));
        v = check_stages(dec & ~STR_ER_WANT_RUN_READ, frames, true, true, true, true);
        CHECK(v.code == STR_ER_EINVAL && names(v));
        v = check_stages(dec & ~STR_ER_WANT_RUN_READ, frames, true, true, false, false);      // (the flag's own rule comes before the table's)
        CHECK(v.code == STR_ER_EINVAL && names(v));
        v = check_stages(grouped | STR_ER_WANT_WORD_DECODE, frames, true, true, true, true);
        CHECK(v.code == STR_ER_EINVAL && names(v));
        v = check_stages(dec, planes, true, true, true, true);
        CHECK(v.code == STR_ER_EINVAL && names(v));
        v = check_stages(dec, strip, true, true, true, true);
        CHECK(v.code == STR_ER_EINVAL && names(v));
        v = check_stages(dec, frames, true, false, false, false);               // (no model either: the model's rule comes before the table's)
        CHECK(v.code == STR_ER_ESTATE && v.msg && std::strstr(v.msg, "STR_ER_WANT_RUN_READ"));
        v = check_stages(dec | STR_ER_WANT_WORD_MATCH, frames, true, true, false, true);      // (both flags: the matcher still needs its lexicon)
        CHECK(v.code == STR_ER_ESTATE && v.msg && std::strstr(v.msg, "STR_ER_WANT_WORD_MATCH"));
        CHECK(check_stages(dec | STR_ER_WANT_WORD_MATCH, frames, true, true, true, true).code == STR_ER_OK);
        // without the flag the table changes no verdict
        for (const uint32_t st : {read, read | STR_ER_WANT_WORD_MATCH, grouped, (uint32_t)STR_ER_STAGE_ALL, read & ~STR_ER_WANT_LINE_WORDS, 0u})
            for (const CallShape &k : {frames, planes, strip})
                for (int cs = 0; cs < 8; ++cs) {
                    const StageVerdict x = check_stages(st, k, cs & 1, cs & 2, cs & 4, false), y = check_stages(st, k, cs & 1, cs & 2, cs & 4, true),
                                       z = check_stages(st, k, cs & 1, cs & 2, cs & 4);
                    CHECK(x.code == y.code && x.msg == y.msg && x.code == z.code && x.msg == z.msg);
                }
        CHECK(STR_ER_WANT_WORD_DECODE == (1u << 23) && STR_ER_WANT_WORD_DECODE == 8388608u);
    }

    std::printf("%ld checks, %ld wrong\n", n_checks, n_wrong);
    return n_wrong ? 1 : 0;
}
