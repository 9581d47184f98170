// Host-only check of csrc/track_read_rules.h (compiled with the host sanitizers and run by tests/test_track_read_host_cpp.py): the
// reading lines, the word links, the word tracks and the track match on random cases against a second, naive statement of the contract
// of str_er_word_link written here (quadratic searches, a closure by relabelling, the recurrence as a full table), and the rules of
// STR_ER_WANT_TRACK_READ in check_stages (csrc/stage_rules.h).  A program of its own; the last line is "<cases> cases <wrong> wrong".
#include "../../scene-text-recognition_amd/csrc/stage_rules.h"
#include "../../scene-text-recognition_amd/csrc/track_read_rules.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace tr = str_er_tr;
namespace wm = str_er_wm;
using namespace str_er_host;

namespace {

long cases = 0, wrong = 0;
#define CHECK(x) do { if (!(x)) { if (++wrong <= 10) std::printf("WRONG line %d: %s\n", __LINE__, #x); } } while (0)

// ---- the naive statement --------------------------------------------------------------------------------------------------------
struct Scene {
    std::vector<str_er_line_foot> feet;
    std::vector<uint32_t>         frame;
    std::vector<int32_t>          track;
    std::vector<int32_t>          wh;
    std::vector<str_er_line_word> words;
};

bool naive_reading(const Scene &s, int t)
{
    for (size_t o = 0; o < s.feet.size(); ++o)
        if ((int)o != t && s.track[o] == s.track[t] && s.frame[o] == s.frame[t] &&
            (s.feet[o].pixels > s.feet[t].pixels || (s.feet[o].pixels == s.feet[t].pixels && (int)o < t)))
            return false;
    return true;
}

int64_t naive_inter(const str_er_line_word &u, const str_er_line_word &v)
{
    int64_t n = 0;          // (the common unit squares, counted one by one)
    for (int64_t x = u.x; x < (int64_t)u.x + u.w; ++x)
        for (int64_t y = u.y; y < (int64_t)u.y + u.h; ++y) n += x >= v.x && x < (int64_t)v.x + v.w && y >= v.y && y < (int64_t)v.y + v.h;
    return n;
}

std::vector<str_er_word_link> naive_links(const Scene &s, int num, int den)
{
    std::vector<str_er_word_link> out;
    for (size_t a = 0; a < s.words.size(); ++a)
        for (size_t b = 0; b < s.words.size(); ++b) {
            const int la = s.words[a].line, lb = s.words[b].line;
            if (!naive_reading(s, la) || !naive_reading(s, lb) || s.track[la] != s.track[lb] || s.frame[lb] != s.frame[la] + 1) continue;
            if (s.wh[2 * s.frame[la]] != s.wh[2 * s.frame[lb]] || s.wh[2 * s.frame[la] + 1] != s.wh[2 * s.frame[lb] + 1]) continue;
            const int64_t inter = naive_inter(s.words[a], s.words[b]);
            if (inter <= 0) continue;
            const int64_t uni = (int64_t)s.words[a].w * s.words[a].h + (int64_t)s.words[b].w * s.words[b].h - inter;
            out.push_back(str_er_word_link{(int32_t)a, (int32_t)b, (uint32_t)inter, inter * den >= (int64_t)num * uni ? 1u : 0u});
        }
    return out;          // (a outer, b inner: sorted by (a, b))
}

// the full table of the recurrence
int32_t naive_cost(const uint8_t *C, int m, const uint8_t *e, int len, int ins, int del, bool fold)
{
    std::vector<std::vector<int64_t>> D((size_t)m + 1, std::vector<int64_t>((size_t)len + 1, 0));
    for (int i = 0; i <= m; ++i) D[(size_t)i][0] = (int64_t)i * del;
    for (int j = 0; j <= len; ++j) D[0][(size_t)j] = (int64_t)j * ins;
    for (int i = 1; i <= m; ++i)
        for (int j = 1; j <= len; ++j) {
            const int a = e[j - 1];
            int       c = C[(size_t)(i - 1) * 65 + a];
            if (fold) c = std::min(c, (int)C[(size_t)(i - 1) * 65 + wm::fold_partner(a)]);
            D[(size_t)i][(size_t)j] = std::min({D[(size_t)i - 1][(size_t)j - 1] + c, D[(size_t)i - 1][(size_t)j] + del, D[(size_t)i][(size_t)j - 1] + ins});
        }
    return (int32_t)D[(size_t)m][(size_t)len];
}

} // namespace

int main()
{
    std::mt19937 rng(12345);
    auto below = [&](int n) { return (int)(rng() % (uint32_t)n); };
    // ---- links and tracks ----
    for (int trial = 0; trial < 700; ++trial) {
        Scene s;
        const int n_frames = 1 + below(5), n_lines = below(12);
        for (int f = 0; f < n_frames; ++f) { s.wh.push_back(below(5) ? 64 : 60); s.wh.push_back(48); }
        for (int t = 0; t < n_lines; ++t) {
            str_er_line_foot F{};
            F.pixels = 10u * (uint32_t)below(4);
            s.feet.push_back(F); s.frame.push_back((uint32_t)below(n_frames)); s.track.push_back(below(3));
            for (int k = below(4); k > 0; --k) s.words.push_back(str_er_line_word{t, 0, 0, below(40), below(6), below(25), below(12), (uint32_t)below(5)});
        }
        const int num = trial % 3 == 0 ? 1 : 1 + below(65535), den = trial % 3 == 0 ? 2 : 1 + below(65535);
        const int n_words = (int)s.words.size();
        std::vector<uint8_t> reading((size_t)n_lines + 1);
        tr::reading_lines(s.feet.data(), s.frame.data(), s.track.data(), n_lines, reading.data());
        for (int t = 0; t < n_lines; ++t) CHECK((reading[(size_t)t] != 0) == naive_reading(s, t));
        std::vector<str_er_word_link> links;
        tr::word_links(s.frame.data(), s.track.data(), reading.data(), n_lines, s.wh.data(), s.words.data(), n_words, num, den, links);
        const std::vector<str_er_word_link> want = naive_links(s, num, den);
        CHECK(links.size() == want.size());
        for (size_t k = 0; k < links.size() && k < want.size(); ++k)
            CHECK(links[k].a == want[k].a && links[k].b == want[k].b && links[k].inter == want[k].inter && links[k].link == want[k].link);
        std::vector<int32_t>           track_of, members;
        std::vector<str_er_word_track> tracks;
        tr::word_tracks(s.frame.data(), s.track.data(), reading.data(), s.words.data(), n_words, links.data(), (int32_t)links.size(), track_of, tracks, members);
        // the closure by relabelling, then every property of the contract one by one
        std::vector<int> comp((size_t)n_words);
        for (int w = 0; w < n_words; ++w) comp[(size_t)w] = w;
        for (const str_er_word_link &L : want)
            if (L.link) {
                const int ca = comp[(size_t)L.a], cb = comp[(size_t)L.b];
                for (int &c : comp) if (c == cb) c = ca;
            }
        CHECK((int)track_of.size() == n_words);
        size_t n_elig = 0;
        for (int w = 0; w < n_words; ++w) {
            const bool elig = naive_reading(s, s.words[(size_t)w].line);
            n_elig += elig;
            CHECK((track_of[(size_t)w] >= 0) == elig);
            for (int v = 0; v < w; ++v)
                if (elig && naive_reading(s, s.words[(size_t)v].line)) CHECK((track_of[(size_t)w] == track_of[(size_t)v]) == (comp[(size_t)w] == comp[(size_t)v]));
        }
        CHECK(members.size() == n_elig);
        int32_t at = 0;
        for (size_t g = 0; g < tracks.size(); ++g) {
            const str_er_word_track &G = tracks[g];
            CHECK(G.first == at && G.count >= 1);
            at += G.count;
            uint32_t f0 = UINT32_MAX, f1 = 0;
            int32_t  rep = -1;
            for (int32_t k = G.first; k < G.first + G.count; ++k) {
                const int32_t w = members[(size_t)k];
                CHECK(track_of[(size_t)w] == (int32_t)g && (k == G.first || members[(size_t)k - 1] < w));
                f0 = std::min(f0, s.frame[(size_t)s.words[(size_t)w].line]); f1 = std::max(f1, s.frame[(size_t)s.words[(size_t)w].line]);
                if (rep < 0 || s.words[(size_t)w].pixels > s.words[(size_t)rep].pixels) rep = w;
                CHECK(G.text_track == s.track[(size_t)s.words[(size_t)w].line]);
            }
            CHECK(G.first_frame == f0 && G.last_frame == f1 && G.rep == rep);
            if (g > 0) {
                const str_er_word_track &P = tracks[g - 1];
                CHECK(P.first_frame < G.first_frame || (P.first_frame == G.first_frame && members[(size_t)P.first] < members[(size_t)G.first]));
            }
        }
        ++cases;
    }
    // ---- the union of bands ----
    for (int m = 0; m <= 40; ++m)
        for (int band = 0; band <= 31; ++band) {
            const uint32_t mask = tr::len_mask_of(m, band);
            for (int l = 1; l <= 32; ++l) CHECK((mask >> (l - 1) & 1u) == (m <= 32 && std::abs(l - m) <= band ? 1u : 0u));
            ++cases;
        }
    // ---- the track match ----
    for (int trial = 0; trial < 400; ++trial) {
        const int            runs_of[] = {0, 1, 2, 3, 5, 8, 9, 16, 17, 32, 33, 36};
        const int            n_words = 1 + below(6);
        std::vector<int32_t> first, n_of;
        int32_t              n_rows = 0;
        for (int w = 0; w < n_words; ++w) { first.push_back(n_rows); n_of.push_back(runs_of[below(trial % 4 ? 7 : 12)]); n_rows += n_of.back(); }
        std::vector<uint8_t> costs((size_t)n_rows * 65 + 1);
        for (uint8_t &c : costs) c = (uint8_t)(below(10) ? 60 + below(196) : below(24));
        const int            n = below(trial % 4 ? 30 : 12);
        std::vector<uint8_t> lab;
        std::vector<int32_t> off{0};
        for (int e = 0; e < n; ++e) {
            for (int k = 1 + below(trial % 4 ? 8 : 32); k > 0; --k) lab.push_back((uint8_t)below(65));
            off.push_back((int32_t)lab.size());
        }
        lab.push_back(0);
        const wm::MatchParams p{1 + below(255), 1 + below(255), below(4) ? below(4) : below(32)};
        const bool            fold = below(2) != 0;
        const int             count = below(7);
        std::vector<int32_t>  members, mc((size_t)count + 1, 12345);
        for (int i = 0; i < count; ++i) members.push_back(below(n_words));
        members.push_back(0);
        const str_er_track_match got = tr::match_track(costs.data(), first.data(), n_of.data(), members.data(), count, lab.data(), off.data(), n, p, fold, mc.data());
        // naive: entry by entry
        int64_t best = -1, bc = -1, second = -1, sc = -1, tried = 0, used = 0, free_c = 0;
        for (int i = 0; i < count; ++i) {
            const int w = members[(size_t)i];
            used += n_of[(size_t)w] <= 32;
            for (int r = 0; r < n_of[(size_t)w]; ++r) free_c += *std::min_element(costs.begin() + ((size_t)first[(size_t)w] + r) * 65, costs.begin() + ((size_t)first[(size_t)w] + r + 1) * 65);
        }
        for (int e = 0; e < n; ++e) {
            const int len = off[(size_t)e + 1] - off[(size_t)e];
            bool      in = false;
            int64_t   sum = 0;
            for (int i = 0; i < count; ++i) {
                const int w = members[(size_t)i], m = n_of[(size_t)w];
                if (m > 32) continue;
                in = in || std::abs(len - m) <= p.band;
                sum += naive_cost(costs.data() + (size_t)first[(size_t)w] * 65, m, lab.data() + off[(size_t)e], len, p.ins, p.del, fold);
            }
            if (!in) continue;
            ++tried;
            if (best < 0 || sum < bc) { second = best; sc = bc; best = e; bc = sum; }
            else if (second < 0 || sum < sc) { second = e; sc = sum; }
        }
        CHECK(got.entry == best && got.cost == bc && got.second_entry == second && got.second_cost == sc);
        CHECK(got.free_cost == free_c && got.n_tried == tried && got.n_used == used);
        int64_t sum = 0, bm = -1;
        for (int i = 0; i < count; ++i) {
            const int w = members[(size_t)i], m = n_of[(size_t)w];
            const int32_t c = best >= 0 && m <= 32 ? naive_cost(costs.data() + (size_t)first[(size_t)w] * 65, m, lab.data() + off[(size_t)best], off[(size_t)best + 1] - off[(size_t)best], p.ins, p.del, fold) : -1;
            CHECK(mc[(size_t)i] == c);
            if (c >= 0) { sum += c; if (bm < 0 || c < mc[(size_t)bm]) bm = i; }
        }
        CHECK(mc[(size_t)count] == 12345);
        CHECK(best < 0 || sum == got.cost);
        CHECK(got.best_member == (bm < 0 ? -1 : members[(size_t)bm]));
        if (count == 1 && n_of[(size_t)members[0]] <= 32) {          // a track of one: the word's own match
            const str_er_word_match w = wm::match_word(costs.data() + (size_t)first[(size_t)members[0]] * 65, n_of[(size_t)members[0]], lab.data(), off.data(), n, p, fold);
            CHECK(w.entry == got.entry && w.cost == got.cost && w.second_entry == got.second_entry && w.second_cost == got.second_cost &&
                  w.free_cost == got.free_cost && w.n_tried == got.n_tried);
        }
        ++cases;
    }
    // ---- the flag's rules ----
    {
        const CallShape frames{true, true, false, false}, planes{false, false, false, false}, strip{false, true, true, false};
        const uint32_t  grouped = STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP,
                        full = grouped | STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_LINKS | STR_ER_WANT_LINE_WORDS | STR_ER_WANT_RUN_READ | STR_ER_WANT_WORD_MATCH |
                               STR_ER_WANT_TRACK_READ;
        CHECK(STR_ER_WANT_TRACK_READ == 33554432u);
        CHECK(check_stages(full, frames, true, true, true, false).code == STR_ER_OK && check_stages(full, frames, true, true, true, false).msg == nullptr);
        CHECK(check_stages(full | STR_ER_WANT_RUN_SPLIT | STR_ER_WANT_WORD_DECODE, frames, true, true, true, true).code == STR_ER_OK);
        const auto names = [](const StageVerdict &v, int code) { return v.code == code && v.msg && std::strstr(v.msg, "STR_ER_WANT_TRACK_READ") == v.msg; };
        CHECK(names(check_stages(full & ~STR_ER_WANT_LINE_LINKS, frames, true, true, true), STR_ER_EINVAL));
        CHECK(names(check_stages(full & ~STR_ER_WANT_WORD_MATCH, frames, true, true, true), STR_ER_EINVAL));
        CHECK(names(check_stages(full & ~STR_ER_WANT_WORD_MATCH, frames, true, true, false), STR_ER_EINVAL));
        CHECK(names(check_stages(full, planes, true, true, true), STR_ER_EINVAL));
        CHECK(names(check_stages(full, strip, true, true, true), STR_ER_EINVAL));
        CHECK(names(check_stages(STR_ER_WANT_TRACK_READ, frames, false, false), STR_ER_EINVAL));
        StageVerdict v = check_stages(full, frames, true, true, false);          // through the matcher: a lexicon
        CHECK(v.code == STR_ER_ESTATE && v.msg && std::strstr(v.msg, "lexicon"));
        v = check_stages(full, frames, true, false, true);                       // ... and through the reading: a model
        CHECK(v.code == STR_ER_ESTATE && v.msg && std::strstr(v.msg, "SVM"));
        cases += 12;
        // without the flag nothing changes: the verdict of every combination of the other bits is the verdict with the bit cleared
        for (uint32_t st = 0; st < (1u << 25); st += 7919)
            for (int cs = 0; cs < 16; ++cs)
                for (const CallShape &k : {frames, planes, strip}) {
                    const StageVerdict x = check_stages(st, k, cs & 1, cs & 2, cs & 4, cs & 8);
                    const StageVerdict y = check_stages(st | STR_ER_WANT_TRACK_READ, k, cs & 1, cs & 2, cs & 4, cs & 8);
                    const bool         riding = !k.strip && k.frames && (st & STR_ER_WANT_LINE_LINKS) && (st & STR_ER_WANT_WORD_MATCH);
                    if (riding) CHECK(x.code == y.code && x.msg == y.msg);
                    else CHECK(names(y, STR_ER_EINVAL));
                }
        ++cases;
    }
    std::printf("%ld cases %ld wrong\n", cases, wrong);
    return wrong ? 1 : 0;
}
