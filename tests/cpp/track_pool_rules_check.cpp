// track_pool_rules_check.cpp -- the rules of the track pool (csrc/track_pool_rules.h, the code the host entry points check with) on the
// CPU, under the host sanitizers: random sequences of add / join / clear on the one-thread pool, every slot read after every step and
// held, field for field, against tr::match_track (rows) and lt::match_track (lattices) on the concatenation of everything the slot was
// given; the widening add, where an accumulation that skips the lengths outside the band misses; the merge of the states; the checks of
// an addition's slots and of a join with the member limit at 65535 / 65536 / 65537.  A program of its own; prints "<checks> checks,
// <wrong> wrong".
#include "../../scene-text-recognition_amd/csrc/track_pool_rules.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace tp = str_er_tp;
namespace lt = str_er_lt;
namespace lm = str_er_lm;
namespace rs = str_er_rs;
namespace tr = str_er_tr;
namespace wm = str_er_wm;

static long n_checks = 0, n_wrong = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++n_checks;                                                                  \
        if (!(cond)) { ++n_wrong; std::printf("line %d: %s\n", __LINE__, #cond); }   \
    } while (0)

struct Words {
    std::vector<str_er_run_split> splits;
    std::vector<uint8_t>          runs, pieces;
    std::vector<int32_t>          first, n_of;
};

template <class Cuts, class Fill> static Words make_words(const std::vector<int> &runs_of, Cuts cuts_of, Fill fill)
{
    Words W;
    int   at = 0;
    for (const int m : runs_of) {
        W.first.push_back((int32_t)W.splits.size());
        W.n_of.push_back(m);
        for (int t = 0; t < m; ++t) {
            const int k = cuts_of();
            W.splits.push_back(str_er_run_split{k, {-1, -1, -1}, 0, at, rs::n_pieces(k), 0});
            at += rs::n_pieces(k);
        }
    }
    W.runs.resize(std::max<size_t>(W.splits.size(), 1) * 65);
    W.pieces.resize((size_t)std::max(at, 1) * 65);
    for (auto &v : W.runs) v = fill();
    for (auto &v : W.pieces) v = fill();
    return W;
}

struct Lexicon {
    std::vector<uint8_t> labels;
    std::vector<int32_t> offsets{0};
    void add(const std::vector<int> &e) { for (const int a : e) labels.push_back((uint8_t)a); offsets.push_back((int32_t)labels.size()); }
    int32_t n() const { return (int32_t)offsets.size() - 1; }
};

static Lexicon random_lexicon(std::mt19937 &rng, int n, int lo, int hi, int labels)
{
    Lexicon X;
    for (int k = 0; k < n; ++k) {
        std::vector<int> e((size_t)(lo + (int)(rng() % (unsigned)(hi - lo + 1))));
        for (int &a : e) a = 65 - labels + (int)(rng() % (unsigned)labels);
        X.add(e);
    }
    return X;
}

// the reference on the concatenated member list, as a pool record with the given member count
static str_er_pool_match reference(const Words &W, const std::vector<int32_t> &members, const Lexicon &X, const lm::Params &p, bool fold, bool lattice)
{
    str_er_track_match t;
    if (lattice) {
        std::vector<str_er_lattice_track_member> mem(members.size() + 1);
        std::vector<uint8_t>                     src(32 * (members.size() + 1));
        std::vector<str_er_split_part>           parts;
        t = lt::match_track(W.splits.data(), W.runs.data(), W.pieces.data(), W.first.data(), W.n_of.data(), members.data(), (int32_t)members.size(), X.labels.data(),
                            X.offsets.data(), X.n(), p, fold, mem.data(), src.data(), parts);
    } else {
        std::vector<int32_t> mc(members.size() + 1);
        t = tr::match_track(W.runs.data(), W.first.data(), W.n_of.data(), members.data(), (int32_t)members.size(), X.labels.data(), X.offsets.data(), X.n(),
                            wm::MatchParams{p.ins, p.del, p.band}, fold, mc.data());
    }
    return str_er_pool_match{t.entry, t.cost, t.second_entry, t.second_cost, t.free_cost, t.n_tried, t.n_used, (int32_t)members.size()};
}

static bool same(const str_er_pool_match &a, const str_er_pool_match &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main()
{
    std::mt19937     rng(11);
    const lm::Params sets[] = {{64, 64, 2, 8}, {1, 1, 0, 0}, {255, 255, 31, 255}, {3, 200, 1, 8}, {2, 2, 2, 1}};
    const auto       cheap = [&] { return (uint8_t)(rng() % 10 == 0 ? rng() % 32 : rng() % 256); };

    // random sequences of add / join / clear: every slot equals the reference on what it was given, after every step
    for (int trial = 0; trial < 48; ++trial) {
        const bool       lattice = trial & 1, fold = trial & 2;
        const lm::Params p = sets[trial % 5];
        const Words      W = lattice ? make_words({0, 1, 2, 3, 5, 9, 12, 2}, [&] { return (int)(rng() % 4); }, cheap)
                                     : make_words({0, 1, 2, 4, 8, 9, 32, 33, 3, 3}, [] { return 0; }, cheap);
        const Lexicon    X = random_lexicon(rng, 70, 1, 12, trial % 3 ? 12 : 4);
        const int32_t    cap = 5, nw = (int32_t)W.first.size();
        tp::Pool         P(cap, X.labels.data(), X.offsets.data(), X.n(), p, fold);
        std::vector<std::vector<int32_t>> given((size_t)cap);
        for (int step = 0; step < 14; ++step) {
            const unsigned op = rng() % 8;
            if (op < 5) {          // add 0 .. 3 members to a slot
                const int32_t        slot = (int32_t)(rng() % cap);
                std::vector<int32_t> mem((size_t)(rng() % 4));
                for (int32_t &w : mem) w = (int32_t)(rng() % (unsigned)nw);
                if (lattice) P.add_lattice(slot, W.splits.data(), W.runs.data(), W.pieces.data(), W.first.data(), W.n_of.data(), mem.data(), (int32_t)mem.size());
                else P.add(slot, W.runs.data(), W.first.data(), W.n_of.data(), mem.data(), (int32_t)mem.size());
                given[(size_t)slot].insert(given[(size_t)slot].end(), mem.begin(), mem.end());
            } else if (op < 7) {   // join one or two other slots into one
                std::vector<int32_t> order(cap);
                for (int32_t i = 0; i < cap; ++i) order[(size_t)i] = i;
                std::shuffle(order.begin(), order.end(), rng);
                const int32_t dst = order[0], n_srcs = 1 + (int32_t)(rng() % 2);
                P.join(dst, order.data() + 1, n_srcs);
                for (int32_t k = 1; k <= n_srcs; ++k) {
                    auto &g = given[(size_t)order[(size_t)k]];
                    given[(size_t)dst].insert(given[(size_t)dst].end(), g.begin(), g.end());
                    g.clear();
                }
            } else {
                const int32_t slot = (int32_t)(rng() % cap);
                P.clear(slot);
                given[(size_t)slot].clear();
            }
            for (int32_t s = 0; s < cap; ++s) {
                std::vector<int32_t> cat = given[(size_t)s];
                CHECK(same(P.read(s), reference(W, cat, X, p, fold, lattice)));
                std::reverse(cat.begin(), cat.end());          // (any order)
                CHECK(same(P.read(s), reference(W, cat, X, p, fold, lattice)));
            }
        }
    }

    // an empty slot reads as a track of no members
    {
        const Lexicon X = random_lexicon(rng, 10, 1, 5, 5);
        tp::Pool      P(2, X.labels.data(), X.offsets.data(), X.n(), sets[0], true);
        CHECK(same(P.read(1), str_er_pool_match{-1, -1, -1, -1, 0, 0, 0, 0}));
    }

    // the widening add at band 0: a member of 3 runs, then one of 7.  The entries of length 7 carry the first member's distance; an
    // accumulation that skips the lengths outside the adding member's band gives another record.
    {
        const Words W = make_words({3, 7}, [] { return 0; }, cheap);
        Lexicon     X;
        for (int k = 0; k < 6; ++k) { std::vector<int> e((size_t)(k < 3 ? 3 : 7)); for (int &a : e) a = (int)(rng() % 65); X.add(e); }
        const lm::Params p{64, 64, 0, 8};
        tp::Pool         P(1, X.labels.data(), X.offsets.data(), X.n(), p, false);
        const int32_t    m0 = 0, m1 = 1;
        P.add(0, W.runs.data(), W.first.data(), W.n_of.data(), &m0, 1);
        CHECK(same(P.read(0), reference(W, {0}, X, p, false, false)) && P.read(0).n_tried == 3);
        P.add(0, W.runs.data(), W.first.data(), W.n_of.data(), &m1, 1);
        const str_er_pool_match want = reference(W, {0, 1}, X, p, false, false);
        CHECK(same(P.read(0), want) && want.n_tried == 6);
        std::vector<int32_t> skip((size_t)X.n(), 0);          // what skipping gives
        for (const int32_t w : {0, 1})
            for (int32_t e = 0; e < X.n(); ++e) {
                const int len = X.offsets[(size_t)e + 1] - X.offsets[(size_t)e];
                if (wm::in_band(W.n_of[(size_t)w], len, p.band))
                    skip[(size_t)e] += wm::entry_cost(W.runs.data() + (size_t)W.first[(size_t)w] * 65, W.n_of[(size_t)w], X.labels.data() + X.offsets[(size_t)e], len, p.ins, p.del, false);
            }
        const str_er_pool_match bad = tp::read_slot(skip.data(), P.st[0], X.offsets.data(), X.n());
        CHECK(bad.cost != want.cost);
    }

    // the merge of the states
    {
        tp::SlotState a{0x5u, 10, 1, 2}, b{0x18u, 7, 3, 4};
        tp::merge(a, b);
        CHECK(a.mask == 0x1Du && a.free_cost == 17 && a.n_used == 4 && a.n_members == 6);
        tp::merge(a, tp::SlotState{});
        CHECK(a.mask == 0x1Du && a.free_cost == 17 && a.n_used == 4 && a.n_members == 6);
    }

    // the member limit and the checks of the slots
    {
        CHECK(tp::members_fit(0, 65536) && tp::members_fit(65535, 1) && !tp::members_fit(65536, 1) && !tp::members_fit(0, 65537) && tp::members_fit(65536, 0));
        std::vector<int32_t> have = {65535, 0, 65536, 1};
        std::vector<uint8_t> seen(4, 0);
        const auto clean = [&] { return std::count(seen.begin(), seen.end(), 0) == 4; };
        const int32_t s01[] = {0, 1}, one[] = {1, 65536}, two[] = {2, 0}, dup[] = {1, 1}, out[] = {0, 4}, neg[] = {-1, 0}, zero[] = {0, 0};
        CHECK(tp::add_check(s01, one, 2, have.data(), 4, seen) == STR_ER_OK && clean());
        CHECK(tp::add_check(s01, two, 2, have.data(), 4, seen) == STR_ER_ECAPACITY && clean());          // 65535 + 2
        const int32_t big[] = {0, 65537};
        CHECK(tp::add_check(s01, big, 2, have.data(), 4, seen) == STR_ER_ECAPACITY && clean());
        CHECK(tp::add_check(dup, zero, 2, have.data(), 4, seen) == STR_ER_EINVAL && clean());
        CHECK(tp::add_check(out, zero, 2, have.data(), 4, seen) == STR_ER_EINVAL && clean());
        CHECK(tp::add_check(neg, zero, 2, have.data(), 4, seen) == STR_ER_EINVAL && clean());
        const int32_t s2[] = {2}, c1[] = {1}, c0[] = {0};
        CHECK(tp::add_check(s2, c1, 1, have.data(), 4, seen) == STR_ER_ECAPACITY && tp::add_check(s2, c0, 1, have.data(), 4, seen) == STR_ER_OK && clean());
        CHECK(tp::add_check(nullptr, nullptr, 0, have.data(), 4, seen) == STR_ER_OK);
        // joins: 65535 + 1 fits, 65535 + 1 + 0 fits, 65536 + 1 does not
        const int32_t j3[] = {3}, j13[] = {1, 3}, j23[] = {2, 3}, j33[] = {3, 3}, j0[] = {0}, j4[] = {4};
        CHECK(tp::join_check(0, j3, 1, have.data(), 4, seen) == STR_ER_OK && clean());
        CHECK(tp::join_check(0, j13, 2, have.data(), 4, seen) == STR_ER_OK && clean());
        CHECK(tp::join_check(0, j23, 2, have.data(), 4, seen) == STR_ER_ECAPACITY && clean());
        CHECK(tp::join_check(2, j3, 1, have.data(), 4, seen) == STR_ER_ECAPACITY && clean());
        CHECK(tp::join_check(1, j33, 2, have.data(), 4, seen) == STR_ER_EINVAL && clean());
        CHECK(tp::join_check(0, j0, 1, have.data(), 4, seen) == STR_ER_EINVAL && clean());
        CHECK(tp::join_check(0, j4, 1, have.data(), 4, seen) == STR_ER_EINVAL && clean());
        CHECK(tp::join_check(4, j3, 1, have.data(), 4, seen) == STR_ER_EINVAL && tp::join_check(-1, j3, 1, have.data(), 4, seen) == STR_ER_EINVAL && clean());
        CHECK(tp::join_check(1, nullptr, 0, have.data(), 4, seen) == STR_ER_OK && clean());
    }

    // 65536 members of one run in one slot: the sums stay inside int32 at the largest cost of a member
    {
        std::vector<uint8_t> rows(65, 255);
        const int32_t        first = 0, n_of = 1;
        Lexicon              X;
        X.add(std::vector<int>(32, 3));
        const lm::Params     p{255, 255, 31, 0};
        tp::Pool             P(1, X.labels.data(), X.offsets.data(), X.n(), p, false);
        std::vector<int32_t> mem((size_t)tr::MAX_MEMBERS, 0);
        P.add(0, rows.data(), &first, &n_of, mem.data(), (int32_t)mem.size());
        const str_er_pool_match r = P.read(0);
        CHECK(r.entry == 0 && r.cost == 65536 * (255 + 31 * 255) && r.n_used == 65536 && r.n_members == 65536 && r.free_cost == 65536 * 255);
    }

    std::printf("%ld checks, %ld wrong\n", n_checks, n_wrong);
    return n_wrong ? 1 : 0;
}
