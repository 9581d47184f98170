// lattice_track_rules_check.cpp -- the rules of the track match over the members' piece lattices (csrc/lattice_track_rules.h, the code
// the host entry point runs) on the CPU, under the host sanitizers: the identities the contract states -- a track of one usable member
// is that word's lattice match (lattice_match_rules.h: match_word), without cuts the record and every member cost are the track match's
// on the runs (track_read_rules.h: match_track) and the parts are the runs, with every member usable it never costs more than the track
// match on the unsplit runs -- the sum of the member costs, the first parts, unusable members, tracks without members, the tie order of
// the backtrack and of best_member on constant rows, the union of bands with a gap, the tracks' checks, the rules of
// STR_ER_WANT_LATTICE_TRACK in check_stages (csrc/stage_rules.h) and the plan of the reading chain with the flag (csrc/read_plan.h) for
// all 256 inputs.  A program of its own; prints "<checks> checks, <wrong> wrong".
#include "../../scene-text-recognition_amd/csrc/lattice_track_rules.h"
#include "../../scene-text-recognition_amd/csrc/read_plan.h"
#include "../../scene-text-recognition_amd/csrc/stage_rules.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

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

// the words of a call: the split records and rows of all runs, and every word's runs
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

struct TrackOut {
    str_er_track_match                       rec;
    std::vector<str_er_lattice_track_member> mem;
    std::vector<uint8_t>                     src;
    std::vector<str_er_split_part>           parts;
};

static TrackOut run_track(const Words &W, const std::vector<int32_t> &members, const Lexicon &X, const lm::Params &p, bool fold)
{
    TrackOut o;
    o.mem.resize(members.size() + 1);
    o.src.assign(32 * (members.size() + 1), 0);
    o.rec = lt::match_track(W.splits.data(), W.runs.data(), W.pieces.data(), W.first.data(), W.n_of.data(), members.data(), (int32_t)members.size(), X.labels.data(),
                            X.offsets.data(), X.n(), p, fold, o.mem.data(), o.src.data(), o.parts);
    return o;
}

static bool same_record(const str_er_track_match &a, const str_er_track_match &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main()
{
    std::mt19937     rng(7);
    const lm::Params sets[] = {{64, 64, 2, 8}, {1, 1, 0, 0}, {255, 255, 31, 255}, {3, 200, 1, 8}, {2, 2, 2, 1}};
    const auto       cheap = [&] { return (uint8_t)(rng() % 10 == 0 ? rng() % 32 : rng() % 256); };
    const auto       small = [&] { return (uint8_t)(rng() % 4); };

    // (1) a track of one member is that word's lattice match
    for (int trial = 0; trial < 60; ++trial) {
        const Words      W = trial % 3 ? make_words({0, 1, 2, 3, 5, 9}, [&] { return (int)(rng() % 4); }, cheap) : make_words({1, 2, 3, 8, 9}, [&] { return (int)(rng() % 4); }, small);
        const Lexicon    X = random_lexicon(rng, 80, 1, 12, trial % 3 ? 12 : 3);
        const lm::Params p = sets[trial % 5];
        const bool       fold = trial & 1;
        for (int32_t w = 0; w < (int32_t)W.first.size(); ++w) {
            const TrackOut     o = run_track(W, {w}, X, p, fold);
            uint8_t            src[32];
            str_er_split_part  parts[lm::MAX_NODES];
            const str_er_lattice_match m = lm::match_word(W.splits.data(), W.runs.data(), W.pieces.data(), W.first[(size_t)w], W.n_of[(size_t)w], X.labels.data(),
                                                          X.offsets.data(), X.n(), p, fold, src, parts);
            const bool usable = lm::word_nodes(W.splits.data(), W.first[(size_t)w], W.n_of[(size_t)w]) <= lm::MAX_NODES;
            CHECK(o.rec.entry == m.entry && o.rec.cost == m.cost && o.rec.second_entry == m.second_entry && o.rec.second_cost == m.second_cost);
            CHECK(o.rec.free_cost == m.free_cost && o.rec.n_tried == m.n_tried && o.rec.n_used == (usable ? 1 : 0));
            CHECK(o.mem[0].word == w && o.mem[0].n_parts == m.n_parts && o.mem[0].n_del == m.n_del && o.mem[0].n_ins == m.n_ins);
            CHECK(o.mem[0].cost == (m.entry >= 0 ? m.cost : -1) && o.rec.best_member == (m.entry >= 0 ? w : -1));
            CHECK(std::memcmp(o.src.data(), src, 32) == 0 && (int32_t)o.parts.size() == m.n_parts);
            CHECK(m.n_parts == 0 || std::memcmp(o.parts.data(), parts, sizeof(str_er_split_part) * (size_t)m.n_parts) == 0);
        }
    }

    // (2) without cuts: the track match on the runs' rows, field for field, and the parts are the runs
    for (int trial = 0; trial < 40; ++trial) {
        const Words      W = make_words({0, 1, 2, 4, 8, 9, 32, 33, 3, 3}, [] { return 0; }, cheap);
        const Lexicon    X = random_lexicon(rng, 100, 1, 10, 10);
        const lm::Params p = sets[trial % 5];
        const bool       fold = trial & 1;
        const std::vector<std::vector<int32_t>> tracks = {{1}, {2, 3, 8}, {0, 4, 5}, {6, 7, 9}, {7}, {8, 9, 8}, {}};
        for (const auto &members : tracks) {
            const TrackOut       o = run_track(W, members, X, p, fold);
            std::vector<int32_t> mc(members.size() + 1);
            const str_er_track_match t = tr::match_track(W.runs.data(), W.first.data(), W.n_of.data(), members.data(), (int32_t)members.size(), X.labels.data(),
                                                         X.offsets.data(), X.n(), wm::MatchParams{p.ins, p.del, p.band}, fold, mc.data());
            CHECK(same_record(o.rec, t));
            size_t at = 0;
            for (size_t i = 0; i < members.size(); ++i) {
                CHECK(o.mem[i].cost == mc[i] && o.mem[i].n_parts == (mc[i] >= 0 ? W.n_of[(size_t)members[i]] : 0));
                for (int32_t k = 0; k < o.mem[i].n_parts; ++k, ++at) CHECK(o.parts[at].run == W.first[(size_t)members[i]] + k && o.parts[at].piece == -1);
            }
            CHECK(at == o.parts.size());
        }
    }

    // (3) every member usable: never more than the track match on the unsplit runs; the member costs add up; counts and sources hold
    for (int trial = 0; trial < 120; ++trial) {
        const bool       ties = trial % 3 == 0;
        const Words      W = ties ? make_words({1, 2, 3, 1, 4}, [&] { return (int)(rng() % 4); }, small) : make_words({1, 2, 3, 1, 4}, [&] { return (int)(rng() % 4); }, cheap);
        const Lexicon    X = random_lexicon(rng, 90, 1, 11, ties ? 3 : 12);
        const lm::Params p = sets[trial % 5];
        const bool       fold = trial & 2;
        std::vector<int32_t> members((size_t)(1 + rng() % 5));
        for (int32_t &w : members) w = (int32_t)(rng() % 5);
        const TrackOut       o = run_track(W, members, X, p, fold);
        std::vector<int32_t> mc(members.size());
        const str_er_track_match t = tr::match_track(W.runs.data(), W.first.data(), W.n_of.data(), members.data(), (int32_t)members.size(), X.labels.data(),
                                                     X.offsets.data(), X.n(), wm::MatchParams{p.ins, p.del, p.band}, fold, mc.data());
        if (t.n_tried > 0) CHECK(o.rec.n_tried >= t.n_tried && o.rec.cost >= 0 && o.rec.cost <= t.cost);
        CHECK(o.rec.n_used == (int32_t)members.size());
        if (o.rec.entry >= 0) {
            const int len = X.offsets[(size_t)o.rec.entry + 1] - X.offsets[(size_t)o.rec.entry];
            int64_t   sum = 0;
            int32_t   best = -1;
            size_t    at = 0;
            for (size_t i = 0; i < members.size(); ++i) {
                const str_er_lattice_track_member &M = o.mem[i];
                lm::Lattice L;
                lm::build(L, W.splits.data(), W.runs.data(), W.pieces.data(), W.first[(size_t)members[i]], W.n_of[(size_t)members[i]]);
                CHECK(M.cost == lm::entry_cost(L, X.labels.data() + X.offsets[(size_t)o.rec.entry], len, p, fold));
                CHECK(M.n_parts - M.n_del + M.n_ins == len && M.n_parts >= L.R && M.n_parts <= L.N);
                sum += M.cost;
                if (best < 0 || M.cost < o.mem[(size_t)best].cost) best = (int32_t)i;
                at += (size_t)M.n_parts;
            }
            CHECK(sum == o.rec.cost && at == o.parts.size() && o.rec.best_member == members[(size_t)best]);
        }
    }

    // unusable members: nothing of theirs is tried, free_cost is still made, their costs are -1
    {
        const Words   W = make_words({33, 9, 2}, [&] { static int k = 0; return k++ < 33 ? 0 : k <= 42 ? 3 : 1; }, cheap);          // N = 33, 36, 4
        const Lexicon X = random_lexicon(rng, 60, 1, 8, 8);
        const lm::Params p = sets[0];
        TrackOut o = run_track(W, {0, 1}, X, p, true);
        CHECK(o.rec.entry == -1 && o.rec.cost == -1 && o.rec.second_entry == -1 && o.rec.n_tried == 0 && o.rec.n_used == 0 && o.rec.best_member == -1);
        CHECK(o.rec.free_cost == lm::free_cost(W.splits.data(), W.runs.data(), W.pieces.data(), 0, 33, p.split) +
                                     lm::free_cost(W.splits.data(), W.runs.data(), W.pieces.data(), 33, 9, p.split));
        CHECK(o.mem[0].cost == -1 && o.mem[1].cost == -1 && o.mem[0].n_parts == 0 && o.parts.empty() && o.src[0] == 0xFF && o.src[63] == 0xFF);
        o = run_track(W, {0, 2, 1}, X, p, true);
        const TrackOut one = run_track(W, {2}, X, p, true);
        CHECK(o.rec.entry == one.rec.entry && o.rec.cost == one.rec.cost && o.rec.n_tried == one.rec.n_tried && o.rec.n_used == 1 && o.rec.best_member == 2);
        CHECK(o.mem[0].cost == -1 && o.mem[2].cost == -1 && o.mem[1].cost == one.mem[0].cost && o.parts.size() == one.parts.size());
        o = run_track(W, {}, X, p, true);
        CHECK(o.rec.entry == -1 && o.rec.free_cost == 0 && o.rec.n_tried == 0 && o.rec.n_used == 0 && o.rec.best_member == -1);
    }

    // the union of bands with a gap: (R, N) = (2, 2) and (10, 14) at band 1 try the lengths 1 .. 3 and 9 .. 15
    {
        const Words W = make_words({2, 10}, [&] { static int k = 0; ++k; return k <= 2 ? 0 : k <= 6 ? 1 : 0; }, [] { return (uint8_t)200; });
        CHECK(lm::word_nodes(W.splits.data(), 0, 2) == 2 && lm::word_nodes(W.splits.data(), 2, 10) == 14);
        CHECK((lt::len_mask_of(2, 2, 1) | lt::len_mask_of(10, 14, 1)) == (0x7u | (0x7Fu << 8)));
        CHECK(lt::len_mask_of(3, 33, 1) == 0 && lt::len_mask_of(0, 0, 0) == 0 && lt::len_mask_of(0, 0, 2) == 0x3u && lt::len_mask_of(40, 32, 31) == (0xFFFFFFu << 8));
        Lexicon X;
        for (const int l : {1, 3, 5, 5, 9, 15, 16, 4}) X.add(std::vector<int>((size_t)l, 7));
        const lm::Params p{1, 1, 1, 0};          // (cheap moves: the entries in the gap would be the cheapest)
        const TrackOut   o = run_track(W, {0, 1}, X, p, false);
        CHECK(o.rec.n_tried == 4 && o.rec.n_used == 2);
        CHECK(o.rec.entry == 0 || o.rec.entry == 1 || o.rec.entry == 4 || o.rec.entry == 5);
    }

    // constant rows: every move costs the same, the order of the candidates decides every part, and the earlier slot is the best member
    {
        const Words W = make_words({1, 1}, [] { return 3; }, [] { return (uint8_t)3; });
        Lexicon     X;
        X.add({5, 6});
        TrackOut o = run_track(W, {1, 0}, X, lm::Params{3, 3, 2, 0}, true);
        CHECK(o.rec.entry == 0 && o.rec.cost == 12 && o.rec.best_member == 1 && o.mem[0].cost == 6 && o.mem[1].cost == 6);
        // at (4, 2) SUB(0) attains 6 (INS at node 0, then the whole run): the smaller i before a later split
        CHECK(o.mem[0].n_parts == 1 && o.mem[0].n_ins == 1 && o.mem[0].n_del == 0 && o.parts.size() == 2 && o.parts[0].run == 1 && o.parts[0].piece == -1 && o.parts[1].run == 0);
        CHECK(o.src[0] == 0x80 && o.src[1] == 0 && o.src[2] == 0xFF && o.src[32] == 0x80 && o.src[33] == 0);
        // with a costly INS the two characters take two parts: the first split the order allows is (0, 1) + (1, 4)
        o = run_track(W, {0, 0}, X, lm::Params{100, 3, 2, 0}, true);
        CHECK(o.rec.cost == 12 && o.rec.best_member == 0 && o.parts.size() == 4 && o.parts[0].piece == W.splits[0].first_piece + rs::piece_index(4, 0, 1) &&
              o.parts[1].piece == W.splits[0].first_piece + rs::piece_index(4, 1, 4) && o.parts[2].piece == o.parts[0].piece && o.src[0] == 0 && o.src[1] == 1);
    }

    // the tracks' checks
    {
        const int32_t first[] = {0, 2}, count[] = {2, 1}, mem[] = {0, 1, 1}, back[] = {2, 0}, over[] = {0, 1};
        CHECK(tr::tracks_check(first, count, mem, 3, 2, 2) == STR_ER_OK);
        CHECK(tr::tracks_check(first, count, mem, 3, 2, 1) == STR_ER_EINVAL);          // a member outside the words
        CHECK(tr::tracks_check(back, count, mem, 3, 2, 2) == STR_ER_EINVAL);           // tracks that do not ascend
        CHECK(tr::tracks_check(over, count, mem, 3, 2, 2) == STR_ER_EINVAL);           // tracks that overlap
        CHECK(tr::tracks_check(first, count, mem, 2, 2, 2) == STR_ER_EINVAL);          // a track outside the member array
        const int32_t f1[] = {0}, big[] = {tr::MAX_MEMBERS + 1};
        std::vector<int32_t> many((size_t)tr::MAX_MEMBERS + 1, 0);
        CHECK(tr::tracks_check(f1, big, many.data(), (int32_t)many.size(), 1, 1) == STR_ER_ECAPACITY);
    }

    // the flag's rules: refused, by name, without any of the flags it rides on and on the strip path and the per-plane calls
    {
        using namespace str_er_host;
        const uint32_t base = STR_ER_STAGE_EXTRACT | STR_ER_STAGE_NMS | STR_ER_STAGE_CLASSIFY | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_WANT_FRAME_LINES |
                              STR_ER_WANT_LINE_WORDS;
        const uint32_t need[] = {STR_ER_WANT_TRACK_READ, STR_ER_WANT_LATTICE_MATCH, STR_ER_WANT_RUN_SPLIT, STR_ER_WANT_WORD_MATCH, STR_ER_WANT_LINE_LINKS, STR_ER_WANT_RUN_READ};
        uint32_t       all = base | STR_ER_WANT_LATTICE_TRACK;
        for (const uint32_t f : need) all |= f;
        const CallShape frames{true, true, false, false}, strip{false, true, true, false}, planes{false, false, false, false};
        CHECK(check_stages(all, frames, true, true, true, false).code == STR_ER_OK);
        CHECK(check_stages(all, frames, true, true, false, false).code == STR_ER_ESTATE);
        for (const uint32_t f : need) {
            const StageVerdict v = check_stages(all & ~f, frames, true, true, true, false);
            CHECK(v.code == STR_ER_EINVAL && v.msg && std::strstr(v.msg, "STR_ER_WANT_LATTICE_TRACK") == v.msg);
        }
        for (const CallShape &k : {strip, planes}) {
            const StageVerdict v = check_stages(all, k, true, true, true, false);
            CHECK(v.code == STR_ER_EINVAL && v.msg && std::strstr(v.msg, "STR_ER_WANT_LATTICE_TRACK") == v.msg);
        }
        // a call without the flag meets no new rule
        for (uint32_t st = 0; st < (1u << 12); ++st) {
            const uint32_t     s = (st & 0x3Fu) | (st >> 6) << 17;          // the stages and the line-stage flags from bit 17 on
            const StageVerdict v = check_stages(s, frames, true, true, true, true);
            CHECK(!v.msg || !std::strstr(v.msg, "STR_ER_WANT_LATTICE_TRACK"));
        }
        // the plan: the lattice track match counts only with the lattice match and the track match, reads set A and changes nothing else
        for (int b = 0; b < 256; ++b) {
            const bool     match = b & 1, decode = b & 2, split = b & 4, lattice = b & 8, track = b & 16, fold = b & 32, lmatch = b & 64, ltrack = b & 128;
            const ReadPlan p = read_plan(match, decode, split, lattice, track, fold, lmatch, ltrack), q = read_plan(match, decode, split, lattice, track, fold, lmatch);
            CHECK(p.ltrack == (ltrack && lmatch && track && split && match) && p.lattice_track_set == (p.ltrack ? SET_A : SET_NONE) && !q.ltrack);
            CHECK(p.rows[0] == q.rows[0] && p.rows[1] == q.rows[1] && p.parts[0] == q.parts[0] && p.parts[1] == q.parts[1] && p.match_set == q.match_set &&
                  p.decode_set == q.decode_set && p.lattice_set == q.lattice_set && p.lattice_match_set == q.lattice_match_set && p.result_set == q.result_set &&
                  p.split_down == q.split_down && p.fold_a == q.fold_a && p.run_probs == q.run_probs && p.lmatch == q.lmatch && p.track == q.track);
            CHECK(!p.ltrack || p.rows[SET_A]);
        }
    }

    std::printf("%ld checks, %ld wrong\n", n_checks, n_wrong);
    return n_wrong ? 1 : 0;
}
