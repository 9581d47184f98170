// decode_pool_rules_check.cpp -- the rules of the decode pool (csrc/decode_pool_rules.h) on the CPU, under the host sanitizers: seeded
// histories of add / join / clear on the one-thread KeepPool for keep = 1, 2, 3, 32, 33, every slot read after every step and held,
// field for field, label for label and cost for cost, against td::decode_track on a list made here from the definition: everything
// usable the slot was ever given, concatenated, sorted by key and cut to the newest `keep`, with the decoder run again on every member.
// Then the groupings of a join: join(0, [1, 2]) against join(0, [1]); join(0, [2]) and join(0, [2]); join(0, [1]).  A program of its own;
// prints "<checks> checks, <wrong> wrong".
#include "../../scene-text-recognition_amd/csrc/decode_pool_rules.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace dp = str_er_dp;
namespace td = str_er_td;
namespace wd = str_er_wd;

static long n_checks = 0, n_wrong = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++n_checks;                                                                  \
        if (!(cond)) { ++n_wrong; std::printf("line %d: %s\n", __LINE__, #cond); }   \
    } while (0)

// what the model remembers of a member: its key and its rows, nothing the pool made
struct Seen {
    uint64_t             key;
    std::vector<uint8_t> rows;          // m x 65
};

struct Params {
    int32_t dec_ins, dec_del, ins, del, rounds;
};

// the record of a slot from the definition
static str_er_pool_decode reference(std::vector<Seen> all, int32_t n_members, int keep, const uint8_t *B, const Params &p, uint8_t *chars, std::vector<int32_t> &mcost)
{
    std::sort(all.begin(), all.end(), [](const Seen &a, const Seen &b) { return a.key < b.key; });
    if ((int)all.size() > keep) all.erase(all.begin(), all.end() - keep);
    const size_t                    n = all.size();
    std::vector<uint8_t>            costs, dchars((n + 1) * wd::MAX_CHARS), src(wd::MAX_CHARS);
    std::vector<int32_t>            first(n + 1), n_of(n + 1), members(n + 1);
    std::vector<str_er_word_decode> dec(n + 1);
    for (size_t i = 0; i < n; ++i) {          // the rows back to back, as a caller of str_er_decode_tracks_host would pass them
        first[i] = (int32_t)(costs.size() / 65);
        n_of[i] = (int32_t)(all[i].rows.size() / 65);
        members[i] = (int32_t)i;
        costs.insert(costs.end(), all[i].rows.begin(), all[i].rows.end());
    }
    costs.resize(costs.size() + 65);
    for (size_t i = 0; i < n; ++i)
        dec[i] = wd::decode_word(costs.data() + (size_t)first[i] * 65, n_of[i], B, p.dec_ins, p.dec_del, dchars.data() + i * wd::MAX_CHARS, src.data());
    mcost.assign((size_t)keep, -1);
    const str_er_track_decode r = td::decode_track(costs.data(), first.data(), n_of.data(), members.data(), (int32_t)n, dec.data(), dchars.data(), B, p.ins, p.del, p.rounds,
                                                   chars, mcost.data());
    return str_er_pool_decode{r.cost, r.seed_cost, r.n_chars, r.n_edits, r.converged, r.n_used, r.seed_member, r.lm_cost, n_members, (int32_t)n};
}

struct Call {
    std::vector<uint8_t> costs;
    std::vector<int32_t> first, n_of, tf, tc, members, slots;
};

// a call of n_tracks tracks on distinct slots, its words of 0 .. 5 rows that read one of a few strings, some of 33 .. 40 rows
static Call make_call(std::mt19937 &rng, int cap, int n_tracks)
{
    Call      c;
    const int n_words = 1 + (int)(rng() % 6);
    for (int w = 0; w < n_words; ++w) {
        const int m = rng() % 7 == 0 ? 33 + (int)(rng() % 8) : (int)(rng() % 6);
        c.first.push_back((int32_t)(c.costs.size() / 65));
        c.n_of.push_back(m);
        for (int i = 0; i < m; ++i)
            for (int a = 0; a < 65; ++a) c.costs.push_back((uint8_t)(a == (int)((i * 7 + w % 2) % 65) ? rng() % 10 : 100 + rng() % 156));
    }
    c.costs.resize(c.costs.size() + 65);
    std::vector<int32_t> order(cap);
    for (int s = 0; s < cap; ++s) order[s] = s;
    std::shuffle(order.begin(), order.end(), rng);
    for (int g = 0; g < n_tracks; ++g) {
        const int count = (int)(rng() % 5);
        c.tf.push_back((int32_t)c.members.size());
        c.tc.push_back(count);
        for (int j = 0; j < count; ++j) c.members.push_back((int32_t)(rng() % n_words));
        if (rng() % 3 == 0) c.members.push_back(0);          // (a slot of the member array that belongs to no track)
        c.slots.push_back(order[g]);
    }
    c.members.push_back(0);
    return c;
}

struct Model {
    std::vector<std::vector<Seen>> all;
    std::vector<int32_t>           n_members;
    uint32_t                       serial = 0;
    explicit Model(int cap) : all((size_t)cap), n_members((size_t)cap, 0) {}
    void add(const Call &c)
    {
        if (c.slots.empty()) return;
        ++serial;
        for (size_t g = 0; g < c.slots.size(); ++g)
            for (int32_t j = 0; j < c.tc[g]; ++j) {
                const int32_t at = c.tf[g] + j, w = c.members[at], m = c.n_of[w];
                ++n_members[c.slots[g]];
                if (m > 32) continue;
                const uint8_t *R = c.costs.data() + (size_t)c.first[w] * 65;
                all[c.slots[g]].push_back(Seen{(uint64_t)serial << 32 | (uint32_t)at, std::vector<uint8_t>(R, R + (size_t)m * 65)});
            }
    }
    void join(int dst, const std::vector<int32_t> &srcs)
    {
        for (const int32_t s : srcs) {
            all[dst].insert(all[dst].end(), all[s].begin(), all[s].end());
            n_members[dst] += n_members[s];
            all[s].clear();
            n_members[s] = 0;
        }
    }
    void clear(int s) { all[s].clear(); n_members[s] = 0; }
};

static void compare(const dp::KeepPool &P, const Model &M, int cap, const uint8_t *B, const Params &p)
{
    for (int s = 0; s < cap; ++s) {
        uint8_t              got_ch[32], want_ch[32];
        std::vector<int32_t> got_mc((size_t)P.keep), want_mc;
        const str_er_pool_decode got = P.read(s, got_ch, got_mc.data()), want = reference(M.all[s], M.n_members[s], P.keep, B, p, want_ch, want_mc);
        CHECK(memcmp(&got, &want, sizeof got) == 0);
        CHECK(memcmp(got_ch, want_ch, 32) == 0);
        CHECK(got_mc == want_mc);
        CHECK(got.n_kept == std::min<int32_t>((int32_t)M.all[s].size(), P.keep) && got.n_used == got.n_kept);
        bool ascending = true;
        for (size_t i = 1; i < P.kept[s].size(); ++i) ascending = ascending && P.kept[s][i - 1].key < P.kept[s][i].key;
        CHECK(ascending);
        if (M.all[s].empty()) CHECK(got.cost == -1 && got.seed_member == -1 && got.n_kept == 0 && got_ch[0] == 0xFF);
    }
}

static void histories(const uint8_t *B)
{
    const int cap = 4;
    for (const int keep : {1, 2, 3, 32, 33})
        for (unsigned seed = 0; seed < 2; ++seed) {
            std::mt19937 rng(1000u * (unsigned)keep + seed);
            const Params p{seed ? 64 : 0, seed ? 64 : 0, 64, 64, keep >= 32 ? 1 : 2};
            dp::KeepPool P(cap, keep, B, p.dec_ins, p.dec_del, p.ins, p.del, p.rounds);
            Model        M(cap);
            const int    steps = keep >= 32 ? 60 : 24;
            for (int step = 0; step < steps; ++step) {
                const unsigned what = rng() % 10;
                if (what < 7) {
                    const Call c = make_call(rng, cap, (int)(rng() % (cap + 1)));
                    P.add(c.costs.data(), c.first.data(), c.n_of.data(), c.tf.data(), c.tc.data(), c.members.data(), (int32_t)c.slots.size(), c.slots.data());
                    M.add(c);
                } else if (what < 9) {
                    std::vector<int32_t> order{0, 1, 2, 3};
                    std::shuffle(order.begin(), order.end(), rng);
                    const int            n_srcs = (int)(rng() % 3);
                    std::vector<int32_t> srcs(order.begin() + 1, order.begin() + 1 + n_srcs);
                    P.join(order[0], srcs.data(), n_srcs);
                    M.join(order[0], srcs);
                } else {
                    const int s = (int)(rng() % cap);
                    P.clear(s);
                    M.clear(s);
                }
                CHECK(P.serial == M.serial);
                if (keep < 32 || step % 4 == 3 || step == steps - 1) compare(P, M, cap, B, p);
            }
            P.reset();
            CHECK(P.serial == 0 && P.kept[0].empty() && P.n_members[1] == 0);
        }
}

static void groupings(const uint8_t *B)
{
    for (const int keep : {1, 2, 3, 32, 33})
        for (unsigned seed = 0; seed < 4; ++seed) {
            const Params p{0, 0, 64, 64, 1};
            dp::KeepPool P[3] = {dp::KeepPool(3, keep, B, 0, 0, 64, 64, 1), dp::KeepPool(3, keep, B, 0, 0, 64, 64, 1), dp::KeepPool(3, keep, B, 0, 0, 64, 64, 1)};
            Model        M(3);
            std::mt19937 rng(77u * (unsigned)keep + seed);
            for (int step = 0; step < (keep >= 32 ? 30 : 6); ++step) {
                const Call c = make_call(rng, 3, 1 + (int)(rng() % 3));
                for (auto &q : P) q.add(c.costs.data(), c.first.data(), c.n_of.data(), c.tf.data(), c.tc.data(), c.members.data(), (int32_t)c.slots.size(), c.slots.data());
                M.add(c);
            }
            const int32_t both[2] = {1, 2}, one[1] = {1}, two[1] = {2};
            P[0].join(0, both, 2);
            P[1].join(0, one, 1); P[1].join(0, two, 1);
            P[2].join(0, two, 1); P[2].join(0, one, 1);
            M.join(0, {1, 2});
            for (auto &q : P) {
                compare(q, M, 3, B, p);
                CHECK(q.kept[0].size() == P[0].kept[0].size() && q.kept[1].empty() && q.kept[2].empty() && q.n_members[0] == M.n_members[0]);
                for (size_t i = 0; i < q.kept[0].size() && i < P[0].kept[0].size(); ++i)
                    CHECK(q.kept[0][i].key == P[0].kept[0][i].key && memcmp(q.kept[0][i].rows, P[0].kept[0][i].rows, dp::CELL_ROW_BYTES) == 0);
            }
        }
}

static void arguments()
{
    CHECK(!dp::create_ok(0, 1) && !dp::create_ok(1, 0) && !dp::create_ok(1, 1025) && dp::create_ok(1, 1) && dp::create_ok(1, 1024));
    CHECK(dp::cells_fit(1 << 14, 1024) && !dp::cells_fit((1 << 14) + 1, 1024) && dp::cells_fit(1 << 24, 1) && !dp::cells_fit((1 << 24) + 1, 1));
    CHECK(dp::make_key(1, 0) == 1ull << 32 && dp::make_key(1, 5) < dp::make_key(2, 0) && dp::make_key(0xFFFFFFFFu, 0x7FFFFFFF) == 0xFFFFFFFF7FFFFFFFull);
    CHECK(dp::usable(0) && dp::usable(32) && !dp::usable(33));
    // the top-keep of a union is the top-keep of the union of top-keeps
    struct K { uint64_t key; };
    std::vector<K> a{{1}, {4}, {9}}, b{{2}, {3}, {10}}, c{{5}, {6}};
    std::vector<K> x = a, y = b;
    dp::merge_keep(x, b, 2); dp::merge_keep(x, c, 2);
    dp::merge_keep(y, c, 2); dp::merge_keep(y, a, 2);
    CHECK(x.size() == 2 && x[0].key == 9 && x[1].key == 10 && y.size() == 2 && y[0].key == 9 && y[1].key == 10);
}

int main()
{
    std::mt19937         rng(5);
    std::vector<uint8_t> B(66 * 66);
    for (auto &v : B) v = (uint8_t)(rng() % 60);
    arguments();
    histories(B.data());
    groupings(B.data());
    std::printf("%ld checks, %ld wrong\n", n_checks, n_wrong);
    return n_wrong == 0 ? 0 : 1;
}
