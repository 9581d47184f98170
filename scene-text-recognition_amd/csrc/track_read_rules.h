// track_read_rules.h -- INTERNAL: the rules of STR_ER_WANT_TRACK_READ (the contract is at str_er_word_link in str_er.h): the reading
// lines of the text tracks, the eligible pairs of words with their common box area and their link, the word tracks as components in
// their order, the union of the members' bands of lengths and the track match of one track on one thread.  HIP-free and header-only,
// on top of word_match_rules.h: the host entry points (api_track_read.cpp), the stage (api_run_read.cpp) and
// tests/cpp/track_read_rules_check.cpp use this same code; track_match_kernels.hip states the match for the device and is held against
// the numpy reference (tests/track_read_ref.py), which is written from the definition.
#pragma once
#include "word_match_rules.h"

#include <algorithm>
#include <numeric>
#include <vector>

namespace str_er_tr {

namespace wm = str_er_wm;

constexpr int MAX_MEMBERS = 65536;        // of one track: 65536 * 64 * 255 stays inside int32

inline bool link_params_ok(int32_t num, int32_t den) { return num >= 1 && num <= 65535 && den >= 1 && den <= 65535; }

// reading[t] = 1 iff line t is R(k, f) of its track k and frame f: the most pixels, a tie stays with the smaller line
inline void reading_lines(const str_er_line_foot *feet, const uint32_t *frames_of_lines, const int32_t *line_tracks, int32_t n_lines, uint8_t *reading)
{
    std::vector<int32_t> order((size_t)n_lines);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int32_t p, int32_t q) {
        if (line_tracks[p] != line_tracks[q]) return line_tracks[p] < line_tracks[q];
        if (frames_of_lines[p] != frames_of_lines[q]) return frames_of_lines[p] < frames_of_lines[q];
        if (feet[p].pixels != feet[q].pixels) return feet[p].pixels > feet[q].pixels;
        return p < q;
    });
    for (int32_t i = 0; i < n_lines; ++i) {
        const int32_t t = order[(size_t)i];
        const bool    head = i == 0 || line_tracks[order[(size_t)i - 1]] != line_tracks[t] || frames_of_lines[order[(size_t)i - 1]] != frames_of_lines[t];
        reading[t] = head ? 1 : 0;
    }
}

inline bool box_ok(const str_er_line_word &w) { return w.w >= 0 && w.w <= 65535 && w.h >= 0 && w.h <= 65535; }
inline uint32_t box_area(const str_er_line_word &w) { return (uint32_t)w.w * (uint32_t)w.h; }

// the area of the intersection of two word boxes (each side at most 65535: it fits)
inline uint32_t box_inter(const str_er_line_word &u, const str_er_line_word &v)
{
    const int64_t x0 = std::max<int64_t>(u.x, v.x), x1 = std::min<int64_t>((int64_t)u.x + u.w, (int64_t)v.x + v.w);
    const int64_t y0 = std::max<int64_t>(u.y, v.y), y1 = std::min<int64_t>((int64_t)u.y + u.h, (int64_t)v.y + v.h);
    return x1 > x0 && y1 > y0 ? (uint32_t)((uint64_t)(x1 - x0) * (uint64_t)(y1 - y0)) : 0u;
}

inline bool link_passes(uint32_t inter, uint32_t au, uint32_t av, int32_t num, int32_t den)
{
    return (uint64_t)inter * (uint64_t)den >= (uint64_t)num * ((uint64_t)au + (uint64_t)av - (uint64_t)inter);
}

// The records of every pair (u of R(k, f), v of R(k, f + 1)) with inter > 0, f and f + 1 adjacent, sorted by (a, b).  The arguments
// are checked by the caller: frames < n_frames, tracks >= 0, words' lines in range, boxes box_ok.
inline void word_links(const uint32_t *frames_of_lines, const int32_t *line_tracks, const uint8_t *reading, int32_t n_lines, const int32_t *frame_wh,
                       const str_er_line_word *words, int32_t n_words, int32_t num, int32_t den, std::vector<str_er_word_link> &out)
{
    out.clear();
    // the words of every reading line, ascending
    std::vector<int32_t> n_of((size_t)n_lines + 1, 0), list((size_t)n_words);
    for (int32_t w = 0; w < n_words; ++w) ++n_of[(size_t)words[w].line + 1];
    for (int32_t t = 0; t < n_lines; ++t) n_of[(size_t)t + 1] += n_of[(size_t)t];
    {
        std::vector<int32_t> at(n_of.begin(), n_of.end() - 1);
        for (int32_t w = 0; w < n_words; ++w) list[(size_t)at[(size_t)words[w].line]++] = w;
    }
    // the reading lines by (track, frame): neighbours in this order are the candidates
    std::vector<int32_t> rl;
    for (int32_t t = 0; t < n_lines; ++t)
        if (reading[t]) rl.push_back(t);
    std::sort(rl.begin(), rl.end(), [&](int32_t p, int32_t q) {
        return line_tracks[p] != line_tracks[q] ? line_tracks[p] < line_tracks[q] : frames_of_lines[p] < frames_of_lines[q];
    });
    for (size_t i = 0; i + 1 < rl.size(); ++i) {
        const int32_t  p = rl[i], q = rl[i + 1];
        const uint32_t f = frames_of_lines[p];
        if (line_tracks[p] != line_tracks[q] || (uint64_t)frames_of_lines[q] != (uint64_t)f + 1u) continue;
        if (frame_wh[2 * (size_t)f] != frame_wh[2 * (size_t)f + 2] || frame_wh[2 * (size_t)f + 1] != frame_wh[2 * (size_t)f + 3]) continue;
        for (int32_t iu = n_of[(size_t)p]; iu < n_of[(size_t)p + 1]; ++iu)
            for (int32_t iv = n_of[(size_t)q]; iv < n_of[(size_t)q + 1]; ++iv) {
                const int32_t  u = list[(size_t)iu], v = list[(size_t)iv];
                const uint32_t inter = box_inter(words[u], words[v]);
                if (inter) out.push_back(str_er_word_link{u, v, inter, link_passes(inter, box_area(words[u]), box_area(words[v]), num, den) ? 1u : 0u});
            }
    }
    std::sort(out.begin(), out.end(), [](const str_er_word_link &x, const str_er_word_link &y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
}

inline int32_t find_root(std::vector<int32_t> &parent, int32_t t)
{
    while (parent[(size_t)t] != t) { parent[(size_t)t] = parent[(size_t)parent[(size_t)t]]; t = parent[(size_t)t]; }
    return t;
}

// The components of the links with link = 1 over the eligible words, ordered by first frame, then by smallest member; members
// ascending; the representative has the most pixels, a tie stays with the smaller word.  track_of[w] = -1 for a word that is not
// eligible.  (checked by the caller: the links join eligible words in range)
inline void word_tracks(const uint32_t *frames_of_lines, const int32_t *line_tracks, const uint8_t *reading, const str_er_line_word *words, int32_t n_words,
                        const str_er_word_link *links, int32_t n_links, std::vector<int32_t> &track_of, std::vector<str_er_word_track> &tracks,
                        std::vector<int32_t> &members)
{
    std::vector<int32_t> parent((size_t)n_words);
    std::iota(parent.begin(), parent.end(), 0);
    for (int32_t k = 0; k < n_links; ++k) {
        if (!links[k].link) continue;
        const int32_t ra = find_root(parent, links[k].a), rb = find_root(parent, links[k].b);
        if (ra != rb) parent[(size_t)std::max(ra, rb)] = std::min(ra, rb);          // (the root is the smallest member)
    }
    const auto frame_of = [&](int32_t w) { return frames_of_lines[words[w].line]; };
    std::vector<uint32_t> f0((size_t)n_words, UINT32_MAX), f1((size_t)n_words, 0);
    std::vector<int32_t>  roots;
    for (int32_t w = 0; w < n_words; ++w) {
        if (!reading[words[w].line]) continue;
        const size_t q = (size_t)find_root(parent, w);
        f0[q] = std::min(f0[q], frame_of(w)); f1[q] = std::max(f1[q], frame_of(w));
        if ((int32_t)q == w) roots.push_back(w);
    }
    std::sort(roots.begin(), roots.end(), [&](int32_t p, int32_t q) { return f0[(size_t)p] != f0[(size_t)q] ? f0[(size_t)p] < f0[(size_t)q] : p < q; });
    std::vector<int32_t> index_of((size_t)n_words, -1);
    tracks.assign(roots.size(), str_er_word_track{});
    for (size_t i = 0; i < roots.size(); ++i) {
        index_of[(size_t)roots[i]] = (int32_t)i;
        tracks[i].first_frame = f0[(size_t)roots[i]]; tracks[i].last_frame = f1[(size_t)roots[i]];
        tracks[i].rep = -1; tracks[i].text_track = line_tracks[words[roots[i]].line];
    }
    track_of.assign((size_t)n_words, -1);
    for (int32_t w = 0; w < n_words; ++w)
        if (reading[words[w].line]) { track_of[(size_t)w] = index_of[(size_t)find_root(parent, w)]; ++tracks[(size_t)track_of[(size_t)w]].count; }
    int32_t at = 0;
    for (str_er_word_track &G : tracks) { G.first = at; at += G.count; G.count = 0; }
    members.assign((size_t)at, 0);
    for (int32_t w = 0; w < n_words; ++w) {
        if (track_of[(size_t)w] < 0) continue;
        str_er_word_track &G = tracks[(size_t)track_of[(size_t)w]];
        members[(size_t)(G.first + G.count++)] = w;
        if (G.rep < 0 || words[w].pixels > words[G.rep].pixels) G.rep = w;
    }
}

// STR_ER_OK, or why not: the tracks ascend in the member array without overlap, the members are words
inline int tracks_check(const int32_t *track_first, const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks, int32_t n_words)
{
    int64_t at = 0;
    for (int32_t g = 0; g < n_tracks; ++g) {
        if (track_count[g] < 0 || track_first[g] < at || (int64_t)track_first[g] + track_count[g] > n_members) return STR_ER_EINVAL;
        if (track_count[g] > MAX_MEMBERS) return STR_ER_ECAPACITY;
        at = (int64_t)track_first[g] + track_count[g];
    }
    for (int32_t i = 0; i < n_members; ++i)
        if (members[i] < 0 || members[i] >= n_words) return STR_ER_EINVAL;
    return STR_ER_OK;
}

// bit l - 1 set iff an entry of length l (1 .. 32) is tried: |l - m| <= band for a usable member
inline uint32_t len_mask_of(int m, int band)
{
    if (m > wm::MAX_LEN) return 0;
    uint32_t mask = 0;
    for (int l = std::max(1, m - band); l <= std::min(wm::MAX_LEN, m + band); ++l) mask |= 1u << (l - 1);
    return mask;
}

// One track against the whole lexicon on one thread: the members are `count` word indices, word w has the rows first_run[w] ..
// first_run[w] + n_of[w] of costs.  member_cost: count values.
inline str_er_track_match match_track(const uint8_t *costs, const int32_t *first_run, const int32_t *n_of, const int32_t *members, int32_t count,
                                      const uint8_t *labels, const int32_t *offsets, int32_t n, const wm::MatchParams &p, bool fold, int32_t *member_cost)
{
    uint32_t mask = 0, free_c = 0;
    int32_t  n_used = 0;
    for (int32_t i = 0; i < count; ++i) {
        const int32_t w = members[i];
        mask |= len_mask_of(n_of[w], p.band);
        n_used += n_of[w] <= wm::MAX_LEN ? 1 : 0;
        free_c += (uint32_t)wm::free_cost(costs + (size_t)first_run[w] * wm::ALPHABET, n_of[w]);
    }
    const auto cost_of = [&](int32_t i, int32_t e) {
        const int32_t w = members[i];
        return wm::entry_cost(costs + (size_t)first_run[w] * wm::ALPHABET, n_of[w], labels + offsets[e], offsets[e + 1] - offsets[e], p.ins, p.del, fold);
    };
    wm::Best2 b;
    int32_t   tried = 0;
    for (int32_t e = 0; e < n; ++e) {
        const int len = offsets[e + 1] - offsets[e];
        if (!(mask >> (len - 1) & 1u)) continue;
        ++tried;
        int32_t sum = 0;
        for (int32_t i = 0; i < count; ++i)
            if (n_of[members[i]] <= wm::MAX_LEN) sum += cost_of(i, e);
        b.add(wm::make_key(sum, e));
    }
    const str_er_word_match r = wm::make_match(b, (int32_t)free_c, tried);
    str_er_track_match      t{r.entry, r.cost, r.second_entry, r.second_cost, r.free_cost, r.n_tried, n_used, -1};
    int32_t                 best = -1;
    for (int32_t i = 0; i < count; ++i) {
        member_cost[i] = t.entry >= 0 && n_of[members[i]] <= wm::MAX_LEN ? cost_of(i, t.entry) : -1;
        if (member_cost[i] >= 0 && (best < 0 || member_cost[i] < member_cost[best])) best = i;
    }
    t.best_member = best < 0 ? -1 : members[best];
    return t;
}

} // namespace str_er_tr
