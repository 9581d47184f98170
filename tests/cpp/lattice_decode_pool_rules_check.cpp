// lattice_decode_pool_rules_check.cpp -- the rules of the lattice decode pool (csrc/lattice_decode_pool_rules.h) on the CPU, under the
// host sanitizers: seeded histories of add / join / clear on the one-thread KeepPool for keep = 1, 2, 3, 32, 33, every slot read after
// every step and held -- record, labels, member costs, member records, sources and parts -- against ltd::decode_track on a list made
// here from the definition, by brute force: everything usable the slot was ever given, concatenated, sorted by key and cut to the newest
// `keep`, every member's runs and pieces gathered again from its call's tables (pieces out of order, foreign pieces in between) and the
// lattice decoder run again on them.  Then the groupings of a join, the rebasing of piece indices and the cells at 72 pieces / 32 runs.
// A program of its own; prints "<checks> checks, <wrong> wrong".
#include "../../scene-text-recognition_amd/csrc/lattice_decode_pool_rules.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace dp = str_er_dp;
namespace ld = str_er_ld;
namespace ldp = str_er_ldp;
namespace lm = str_er_lm;
namespace ltd = str_er_ltd;
namespace rs = str_er_rs;

static long n_checks = 0, n_wrong = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++n_checks;                                                                  \
        if (!(cond)) { ++n_wrong; std::printf("line %d: %s\n", __LINE__, #cond); }   \
    } while (0)

// what the model remembers of a member: its key, its runs' cut counts and its rows in lattice order, nothing the pool made
struct Seen {
    uint64_t                          key;
    std::vector<int32_t>              cuts;            // per run
    std::vector<std::vector<uint8_t>> run_rows;        // per run: 65 bytes
    std::vector<std::vector<uint8_t>> piece_rows;      // per run: n_pieces x 65 bytes
};

struct Params {
    int32_t dec_ins, dec_del, ins, del, rounds, split;
};

// the read of a slot from the definition: the kept list laid out densely (runs and pieces back to back, no cell strides), decoded, and
// its parts translated to the strides of the contract
static ldp::Read reference(std::vector<Seen> all, int32_t n_members, int keep, const uint8_t *B, const Params &p)
{
    std::sort(all.begin(), all.end(), [](const Seen &a, const Seen &b) { return a.key < b.key; });
    if ((int)all.size() > keep) all.erase(all.begin(), all.end() - keep);
    const size_t                       n = all.size();
    std::vector<str_er_run_split>      splits;
    std::vector<uint8_t>               rr, pr, dchars((n + 1) * ld::MAX_CHARS), src(ld::MAX_CHARS);
    std::vector<int32_t>               first(n + 1), n_of(n + 1), members(n + 1), run0(n + 1), piece0(n + 1);
    std::vector<str_er_lattice_decode> dec(n + 1);
    for (size_t i = 0; i < n; ++i) {
        first[i] = run0[i] = (int32_t)splits.size();
        piece0[i] = (int32_t)(pr.size() / 65);
        n_of[i] = (int32_t)all[i].cuts.size();
        members[i] = (int32_t)i;
        for (size_t t = 0; t < all[i].cuts.size(); ++t) {
            str_er_run_split S{};
            S.n_cuts = all[i].cuts[t];
            S.n_pieces = rs::n_pieces(S.n_cuts);
            S.first_piece = (int32_t)(pr.size() / 65);
            S.cut[0] = S.cut[1] = S.cut[2] = -1;
            splits.push_back(S);
            rr.insert(rr.end(), all[i].run_rows[t].begin(), all[i].run_rows[t].end());
            pr.insert(pr.end(), all[i].piece_rows[t].begin(), all[i].piece_rows[t].end());
        }
    }
    splits.push_back(str_er_run_split{});
    rr.resize(rr.size() + 65); pr.resize(pr.size() + 65);
    str_er_split_part dparts[ld::MAX_NODES + 1];
    for (size_t i = 0; i < n; ++i)
        dec[i] = ld::decode_word(splits.data(), rr.data(), pr.data(), first[i], n_of[i], B, p.dec_ins, p.dec_del, p.split, dchars.data() + i * ld::MAX_CHARS, src.data(), dparts);
    ldp::Read R;
    R.members.assign(n + 1, str_er_lattice_track_member{-1, 0, 0, 0, 0, -1});
    R.src.assign((n + 1) * lm::SRC_BYTES, 0xFF);
    const lm::Params          q{p.ins, p.del, 0, p.split};
    const str_er_track_decode r = ltd::decode_track(splits.data(), rr.data(), pr.data(), first.data(), n_of.data(), members.data(), (int32_t)n, dec.data(), dchars.data(), B, q,
                                                    p.rounds, R.chars, R.members.data(), R.src.data(), R.parts);
    R.members.resize(n);
    R.src.resize(n * lm::SRC_BYTES);
    R.member_cost.assign((size_t)keep, -1);
    int32_t fp = 0;
    for (size_t i = 0; i < n; ++i) {
        R.member_cost[i] = R.members[i].cost;
        R.members[i].first_part = fp;
        for (int32_t k = 0; k < R.members[i].n_parts; ++k) {          // dense indices -> 32 * rank + run, 80 * rank + piece row
            str_er_split_part &P = R.parts[(size_t)(fp + k)];
            P.run = P.run - run0[i] + (int32_t)i * ldp::CELL_RUNS;
            if (P.piece >= 0) P.piece = P.piece - piece0[i] + (int32_t)i * ldp::CELL_PIECES;
        }
        fp += R.members[i].n_parts;
    }
    R.rec = str_er_pool_decode{r.cost, r.seed_cost, r.n_chars, r.n_edits, r.converged, r.n_used, r.seed_member, r.lm_cost, n_members, (int32_t)n};
    return R;
}

struct Call {
    std::vector<str_er_run_split> splits;
    std::vector<uint8_t>          rr, pr;
    std::vector<int32_t>          first, n_of, tf, tc, members, slots;
};

static void random_row(std::mt19937 &rng, std::vector<uint8_t> &to, int like)
{
    for (int a = 0; a < 65; ++a) to.push_back((uint8_t)(a == like % 65 ? rng() % 10 : 60 + rng() % 196));
}

// a word of the given cut counts into the call; its runs' pieces lie in the piece table in reverse run order, foreign rows between them
static void push_word(std::mt19937 &rng, Call &c, const std::vector<int> &cuts)
{
    c.first.push_back((int32_t)c.splits.size());
    c.n_of.push_back((int32_t)cuts.size());
    const size_t r0 = c.splits.size();
    for (size_t t = 0; t < cuts.size(); ++t) {
        str_er_run_split S{};
        S.n_cuts = cuts[t];
        S.n_pieces = rs::n_pieces(cuts[t]);
        S.cut[0] = S.cut[1] = S.cut[2] = -1;
        c.splits.push_back(S);
        random_row(rng, c.rr, (int)(t * 7 + cuts.size()));
    }
    for (size_t t = cuts.size(); t-- > 0;) {
        for (unsigned k = rng() % 3; k > 0; --k) random_row(rng, c.pr, 0);          // foreign pieces
        c.splits[r0 + t].first_piece = (int32_t)(c.pr.size() / 65);
        for (int k = 0; k < c.splits[r0 + t].n_pieces; ++k) random_row(rng, c.pr, (int)(t * 7 + k + 1));
    }
}

// a call of n_tracks tracks on distinct slots, its words of 0 .. 4 runs with 0 .. 3 cuts, some of 33 nodes and more
static Call make_call(std::mt19937 &rng, int cap, int n_tracks)
{
    Call      c;
    const int n_words = 1 + (int)(rng() % 6);
    for (int w = 0; w < n_words; ++w) {
        std::vector<int> cuts;
        if (rng() % 7 == 0) cuts.assign(9 + rng() % 3, 3);          // 36 nodes and more: unusable
        else
            for (unsigned k = rng() % 5; k > 0; --k) cuts.push_back((int)(rng() % 4));
        push_word(rng, c, cuts);
    }
    c.splits.push_back(str_er_run_split{});
    c.rr.resize(c.rr.size() + 65); c.pr.resize(c.pr.size() + 65);
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

static Seen see(const Call &c, uint64_t key, int32_t w)
{
    Seen s{key, {}, {}, {}};
    for (int32_t t = 0; t < c.n_of[w]; ++t) {
        const str_er_run_split &S = c.splits[(size_t)(c.first[w] + t)];
        s.cuts.push_back(S.n_cuts);
        const uint8_t *R = c.rr.data() + (size_t)(c.first[w] + t) * 65, *P = c.pr.data() + (size_t)S.first_piece * 65;
        s.run_rows.emplace_back(R, R + 65);
        s.piece_rows.emplace_back(P, P + (size_t)S.n_pieces * 65);
    }
    return s;
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
                const int32_t at = c.tf[g] + j, w = c.members[at];
                ++n_members[c.slots[g]];
                int N = 0;
                for (int32_t t = 0; t < c.n_of[w]; ++t) N += c.splits[(size_t)(c.first[w] + t)].n_cuts + 1;
                if (N > 32) continue;
                all[c.slots[g]].push_back(see(c, (uint64_t)serial << 32 | (uint32_t)at, w));
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

static bool same_read(const ldp::Read &a, const ldp::Read &b)
{
    return memcmp(&a.rec, &b.rec, sizeof a.rec) == 0 && memcmp(a.chars, b.chars, ltd::MAX_LEN) == 0 && a.member_cost == b.member_cost && a.src == b.src &&
           a.members.size() == b.members.size() && (a.members.empty() || memcmp(a.members.data(), b.members.data(), a.members.size() * sizeof a.members[0]) == 0) &&
           a.parts.size() == b.parts.size() && (a.parts.empty() || memcmp(a.parts.data(), b.parts.data(), a.parts.size() * sizeof a.parts[0]) == 0);
}

static void add(ldp::KeepPool &P, const Call &c)
{
    P.add(c.splits.data(), c.rr.data(), c.pr.data(), c.first.data(), c.n_of.data(), c.tf.data(), c.tc.data(), c.members.data(), (int32_t)c.slots.size(), c.slots.data());
}

static void compare(const ldp::KeepPool &P, const Model &M, int cap, const uint8_t *B, const Params &p)
{
    for (int s = 0; s < cap; ++s) {
        const ldp::Read got = P.read(s), want = reference(M.all[s], M.n_members[s], P.keep, B, p);
        CHECK(same_read(got, want));
        CHECK(got.rec.n_kept == std::min<int32_t>((int32_t)M.all[s].size(), P.keep) && got.rec.n_used == got.rec.n_kept);
        bool ascending = true, words = true;
        for (size_t i = 1; i < P.kept[s].size(); ++i) ascending = ascending && P.kept[s][i - 1].key < P.kept[s][i].key;
        for (size_t i = 0; i < got.members.size(); ++i) words = words && got.members[i].word == (int32_t)i;
        CHECK(ascending && words);
        if (M.all[s].empty()) CHECK(got.rec.cost == -1 && got.rec.seed_member == -1 && got.rec.n_kept == 0 && got.chars[0] == 0xFF && got.parts.empty());
    }
}

static void histories(const uint8_t *B)
{
    const int cap = 4;
    for (const int keep : {1, 2, 3, 32, 33})
        for (unsigned seed = 0; seed < 2; ++seed) {
            std::mt19937 rng(1000u * (unsigned)keep + seed);
            const Params p{seed ? 64 : 0, seed ? 64 : 0, 64, 64, keep >= 32 ? 1 : 2, seed ? 0 : 8};
            ldp::KeepPool P(cap, keep, B, p.dec_ins, p.dec_del, p.ins, p.del, p.rounds, p.split);
            Model         M(cap);
            const int     steps = keep >= 32 ? 40 : 24;
            for (int step = 0; step < steps; ++step) {
                const unsigned what = rng() % 10;
                if (what < 7) {
                    const Call c = make_call(rng, cap, (int)(rng() % (cap + 1)));
                    add(P, c);
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
        for (unsigned seed = 0; seed < 3; ++seed) {
            const Params  p{0, 0, 64, 64, 1, 8};
            ldp::KeepPool P[3] = {ldp::KeepPool(3, keep, B, 0, 0, 64, 64, 1, 8), ldp::KeepPool(3, keep, B, 0, 0, 64, 64, 1, 8), ldp::KeepPool(3, keep, B, 0, 0, 64, 64, 1, 8)};
            Model         M(3);
            std::mt19937  rng(77u * (unsigned)keep + seed);
            for (int step = 0; step < (keep >= 32 ? 20 : 6); ++step) {
                const Call c = make_call(rng, 3, 1 + (int)(rng() % 3));
                for (auto &q : P) add(q, c);
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
                    CHECK(q.kept[0][i].key == P[0].kept[0][i].key && memcmp(q.kept[0][i].run_rows, P[0].kept[0][i].run_rows, ldp::CELL_RUN_BYTES) == 0 &&
                          memcmp(q.kept[0][i].piece_rows, P[0].kept[0][i].piece_rows, ldp::CELL_PIECE_BYTES) == 0 &&
                          memcmp(q.kept[0][i].splits, P[0].kept[0][i].splits, ldp::CELL_SPLIT_BYTES) == 0);
            }
        }
}

// the cells at their limits and the rebasing rule on them: 8 runs of 3 cuts (72 pieces, 32 nodes), 32 uncut runs, and one node more
static void cells(const uint8_t *B)
{
    std::mt19937 rng(9);
    Call         c;
    push_word(rng, c, std::vector<int>(8, 3));
    push_word(rng, c, std::vector<int>(32, 0));
    std::vector<int> over(8, 3);
    over.push_back(0);
    push_word(rng, c, over);
    push_word(rng, c, {2, 0, 1});
    c.splits.push_back(str_er_run_split{});
    c.rr.resize(c.rr.size() + 65); c.pr.resize(c.pr.size() + 65);
    c.tf = {0}; c.tc = {5}; c.members = {0, 1, 2, 3, 0}; c.slots = {0};
    const Params  p{0, 0, 64, 64, 1, 8};
    ldp::KeepPool P(1, 8, B, 0, 0, 64, 64, 1, 8);
    Model         M(1);
    add(P, c);
    M.add(c);
    compare(P, M, 1, B, p);
    CHECK(P.kept[0].size() == 4 && P.n_members[0] == 5);
    CHECK(ldp::usable(c.splits.data(), c.first[0], c.n_of[0]) && ldp::usable(c.splits.data(), c.first[1], c.n_of[1]) && !ldp::usable(c.splits.data(), c.first[2], c.n_of[2]));
    for (const ldp::Member &m : P.kept[0]) {
        int32_t base = 0;
        for (int32_t t = 0; t < m.n_runs; ++t) {          // the pieces back to back in run order, each row the call's
            CHECK(m.splits[t].first_piece == base && ldp::piece_base(m.splits, t) == base);
            base += m.splits[t].n_pieces;
        }
        CHECK(base <= ldp::CELL_PIECES_USED && m.n_runs <= ldp::CELL_RUNS);
        for (int32_t t = m.n_runs; t < ldp::CELL_RUNS; ++t) CHECK(m.splits[t].n_cuts == 0 && m.splits[t].n_pieces == 0);
    }
    const ldp::Member &full = P.kept[0][0];
    CHECK(full.n_runs == 8 && ldp::piece_base(full.splits, 8) == 72);
    for (int32_t t = 0; t < 8; ++t) {
        const str_er_run_split &S = c.splits[(size_t)(c.first[0] + t)];
        CHECK(memcmp(full.piece_rows + (size_t)full.splits[t].first_piece * 65, c.pr.data() + (size_t)S.first_piece * 65, 9 * 65) == 0);
        CHECK(memcmp(full.run_rows + (size_t)t * 65, c.rr.data() + (size_t)(c.first[0] + t) * 65, 65) == 0);
        const str_er_run_split R = ldp::rebased(S, 80 * 5, ldp::piece_base(c.splits.data() + c.first[0], t));
        CHECK(R.first_piece == 400 + 9 * t && R.n_cuts == S.n_cuts && R.n_pieces == S.n_pieces && R.thr == S.thr && R.cut[0] == S.cut[0] && R.n_parts == S.n_parts);
    }
    // a read's parts index the strides: run 32 * rank + t, piece 80 * rank + row
    const ldp::Read got = P.read(0);
    for (size_t i = 0; i < got.members.size(); ++i)
        for (int32_t k = 0; k < got.members[i].n_parts; ++k) {
            const str_er_split_part &q = got.parts[(size_t)(got.members[i].first_part + k)];
            CHECK(q.run >= 32 * (int32_t)i && q.run < 32 * (int32_t)i + P.kept[0][i].n_runs && (q.piece == -1 || (q.piece >= 80 * (int32_t)i && q.piece < 80 * (int32_t)i + 72)));
        }
}

static void arguments()
{
    CHECK(!ldp::create_ok(0, 1) && !ldp::create_ok(1, 0) && !ldp::create_ok(1, 1025) && ldp::create_ok(1, 1) && ldp::create_ok(1, 1024));
    // 80 piece rows a cell, all below 2^30 (the flag of a piece's row in the structure table): 13 421 772 cells, fewer than the decode pool's 2^24
    CHECK(ldp::MAX_CELLS == 13421772 && 80 * ldp::MAX_CELLS <= (1ll << 30) && 80 * (ldp::MAX_CELLS + 1) > (1ll << 30) && ldp::MAX_CELLS < dp::MAX_CELLS);
    CHECK(ldp::cells_fit(13421772, 1) && !ldp::cells_fit(13421773, 1) && ldp::cells_fit(13107, 1024) && !ldp::cells_fit(13108, 1024) && !ldp::cells_fit(1 << 14, 1024) &&
          !ldp::cells_fit(1 << 24, 1));
    CHECK(ldp::CELL_BYTES == 9072 && ldp::CELL_RUN_BYTES == 2080 && ldp::CELL_PIECE_BYTES == 5200 && ldp::CELL_SPLIT_BYTES == 1024 && ldp::TAB_BYTES == 656);
    CHECK((int64_t)ldp::CELL_BYTES * ldp::MAX_CELLS < ldp::MAX_STORE_BYTES);          // (the cell bound is the tighter one)
}

int main()
{
    std::mt19937         rng(5);
    std::vector<uint8_t> B(66 * 66);
    for (auto &v : B) v = (uint8_t)(rng() % 60);
    arguments();
    cells(B.data());
    histories(B.data());
    groupings(B.data());
    std::printf("%ld checks, %ld wrong\n", n_checks, n_wrong);
    return n_wrong == 0 ? 0 : 1;
}
