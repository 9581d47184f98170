// Host-only check of csrc/lines_host.cpp (compiled with it alone under -fsanitize=address,undefined and run by
// tests/test_lines_host_cpp.py): str_er_frame_lines_from_pairs and str_er_text_tracks_from_links on the hand-made cases of the two
// _abi tests, with their results written out, and on random small cases against a brute-force partition (a reachability matrix: no
// union-find, no code of lines_host.cpp); str_er_hull_of_points and str_er_quad_from_hull on the degenerate sets, at the corners of
// the coordinate range and on random sets against an O(n^3) hull and an O(n^2) smallest box.  Every array the functions write lies
// at the end of a heap block of exactly its size, so that a write past an end is the sanitizer's to find.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <memory>
#include <utility>
#include <vector>

#include "../../include/str_er.h"

namespace {

long bad = 0, cases = 0;

void expect(bool ok, const char *what, long k = -1)
{
    ++cases;
    if (ok) return;
    if (++bad <= 10) printf("WRONG: %s (%ld)\n", what, k);
}

uint64_t lcg_state = 20261018u;
uint32_t lcg() { lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(lcg_state >> 33); }
int32_t  below(uint32_t n) { return (int32_t)(lcg() % n); }

template <typename T> std::unique_ptr<T[]> block(const std::vector<T> &v)          // exactly v.size() records
{
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

typedef __int128 i128;
struct Pt { int32_t x, y; };
bool operator==(const Pt &a, const Pt &b) { return a.x == b.x && a.y == b.y; }
bool before(const Pt &a, const Pt &b) { return a.y != b.y ? a.y < b.y : a.x < b.x; }
i128 cross(const Pt &o, const Pt &a, const Pt &b) { return (i128)((int64_t)a.x - o.x) * ((int64_t)b.y - o.y) - (i128)((int64_t)a.y - o.y) * ((int64_t)b.x - o.x); }

// ---- the partitions --------------------------------------------------------------------------------------------------------------------

struct Edge { int32_t a, b; uint32_t inter; uint32_t flag; };         // (flag: a pair's dup as given)

bool passes(uint32_t inter, uint32_t pa, uint32_t pb, int32_t num, int32_t den)
{
    return (i128)inter * den >= (i128)num * ((i128)pa + pb - inter);
}

struct Group { uint32_t key, key1; int32_t rep; uint32_t pixels; std::vector<int32_t> members; };

// the components of the joined edges by reachability, ordered by (key of the component, smallest member); key: the smallest frame
std::vector<Group> partition(const std::vector<uint32_t> &pixels, const std::vector<uint32_t> &frames, const std::vector<std::pair<int32_t, int32_t>> &joined,
                             std::vector<int32_t> &group_of)
{
    const size_t n = pixels.size();
    std::vector<std::vector<char>> reach(n, std::vector<char>(n, 0));
    for (size_t i = 0; i < n; ++i) reach[i][i] = 1;
    for (const auto &e : joined) reach[(size_t)e.first][(size_t)e.second] = reach[(size_t)e.second][(size_t)e.first] = 1;
    for (size_t k = 0; k < n; ++k)
        for (size_t i = 0; i < n; ++i)
            for (size_t j = 0; j < n; ++j)
                if (reach[i][k] && reach[k][j]) reach[i][j] = 1;
    std::vector<Group> groups;
    for (size_t i = 0; i < n; ++i) {
        bool smallest = true;
        for (size_t j = 0; j < i; ++j) smallest = smallest && !reach[i][j];
        if (!smallest) continue;
        Group g{UINT32_MAX, 0, -1, 0, {}};
        for (size_t j = i; j < n; ++j) {
            if (!reach[i][j]) continue;
            g.members.push_back((int32_t)j);
            g.key = std::min(g.key, frames[j]); g.key1 = std::max(g.key1, frames[j]);
            if (g.rep < 0 || pixels[j] > g.pixels) { g.rep = (int32_t)j; g.pixels = pixels[j]; }
        }
        groups.push_back(g);
    }
    std::stable_sort(groups.begin(), groups.end(), [](const Group &p, const Group &q) { return p.key < q.key; });         // (they were in order of their smallest member)
    group_of.assign(n, -1);
    for (size_t g = 0; g < groups.size(); ++g)
        for (const int32_t m : groups[g].members) group_of[(size_t)m] = (int32_t)g;
    return groups;
}

struct Box { int32_t x, y, w, h; };

struct PairsCall {
    int rc = 0, rc_count = 0, rc_small = 0;
    int32_t n = -1, n_count = -1;
    std::vector<str_er_line_foot> feet;
    std::vector<str_er_line_pair> pairs;
    std::vector<str_er_frame_line> lines;
    std::vector<int32_t> members;
};

// the counting call, the call with exactly as many records as needed, and the call with one record less
PairsCall from_pairs(const std::vector<Box> &boxes, const std::vector<uint32_t> &pixels, const std::vector<uint32_t> &frames, const std::vector<uint8_t> &pyr,
                     const std::vector<Edge> &edges, int32_t num, int32_t den)
{
    PairsCall c;
    const int32_t n = (int32_t)pixels.size();
    std::vector<str_er_line_foot> ft;
    for (int32_t t = 0; t < n; ++t) ft.push_back(str_er_line_foot{boxes[(size_t)t].x, boxes[(size_t)t].y, boxes[(size_t)t].w, boxes[(size_t)t].h, pixels[(size_t)t], -7});
    std::vector<str_er_line_pair> pr;
    for (const Edge &e : edges) pr.push_back(str_er_line_pair{e.a, e.b, e.inter, 9u});
    auto feet = block(ft);
    auto pairs = block(pr);
    auto fr = block(frames);
    auto py = block(pyr);
    c.rc_count = str_er_frame_lines_from_pairs(feet.get(), fr.get(), py.get(), n, pairs.get(), (int32_t)pr.size(), num, den, nullptr, 0, &c.n_count, nullptr);
    if (c.rc_count != STR_ER_OK) { c.rc = c.rc_count; return c; }
    std::unique_ptr<str_er_frame_line[]> lines(new str_er_frame_line[(size_t)c.n_count]);
    std::unique_ptr<int32_t[]> members(new int32_t[(size_t)n]);
    c.rc = str_er_frame_lines_from_pairs(feet.get(), fr.get(), py.get(), n, pairs.get(), (int32_t)pr.size(), num, den, lines.get(), c.n_count, &c.n, members.get());
    c.feet.assign(feet.get(), feet.get() + n);
    c.pairs.assign(pairs.get(), pairs.get() + pr.size());
    c.lines.assign(lines.get(), lines.get() + c.n_count);
    c.members.assign(members.get(), members.get() + n);
    if (c.n_count > 0) {
        std::unique_ptr<str_er_frame_line[]> few(new str_er_frame_line[(size_t)c.n_count - 1]);
        int32_t got = -1;
        c.rc_small = str_er_frame_lines_from_pairs(feet.get(), fr.get(), py.get(), n, pairs.get(), (int32_t)pr.size(), num, den, few.get(), c.n_count - 1, &got, members.get());
        if (got != c.n_count) c.rc_small = 1000;
    } else c.rc_small = STR_ER_ECAPACITY;
    return c;
}

void agree_pairs(const std::vector<Box> &boxes, const std::vector<uint32_t> &pixels, const std::vector<uint32_t> &frames, const std::vector<uint8_t> &pyr,
                 const std::vector<Edge> &edges, int32_t num, int32_t den, long k)
{
    const PairsCall c = from_pairs(boxes, pixels, frames, pyr, edges, num, den);
    std::vector<std::pair<int32_t, int32_t>> joined;
    bool ok = c.rc == STR_ER_OK && c.rc_count == STR_ER_OK && c.rc_small == STR_ER_ECAPACITY;
    for (size_t i = 0; ok && i < edges.size(); ++i) {
        const bool dup = passes(edges[i].inter, pixels[(size_t)edges[i].a], pixels[(size_t)edges[i].b], num, den);
        ok = c.pairs[i].dup == (dup ? 1u : 0u) && c.pairs[i].a == edges[i].a && c.pairs[i].b == edges[i].b && c.pairs[i].inter == edges[i].inter;
        if (dup) joined.push_back({edges[i].a, edges[i].b});
    }
    expect(ok, "from_pairs: codes, counting mode, capacity and dup", k);
    if (!ok) return;
    std::vector<int32_t> group_of;
    const std::vector<Group> groups = partition(pixels, frames, joined, group_of);
    ok = c.n == (int32_t)groups.size() && c.n_count == c.n;
    int32_t at = 0;
    for (size_t g = 0; ok && g < groups.size(); ++g) {
        const Group &G = groups[g];
        const str_er_frame_line &F = c.lines[g];
        uint32_t levels = 0;
        int32_t x0 = 0, y0 = 0, x1 = 0, y1 = 0;
        bool any = false;
        for (const int32_t m : G.members) {
            if (pyr[(size_t)m] < 32) levels |= 1u << pyr[(size_t)m];
            const Box &B = boxes[(size_t)m];
            if (B.w <= 0 || B.h <= 0) continue;
            x0 = any ? std::min(x0, B.x) : B.x; y0 = any ? std::min(y0, B.y) : B.y;
            x1 = any ? std::max(x1, B.x + B.w) : B.x + B.w; y1 = any ? std::max(y1, B.y + B.h) : B.y + B.h;
            any = true;
        }
        ok = F.frame == G.key && F.rep == G.rep && F.pixels == G.pixels && F.first == at && F.count == (int32_t)G.members.size() && F.levels == levels &&
             F.x == x0 && F.y == y0 && F.w == x1 - x0 && F.h == y1 - y0;
        for (size_t i = 0; ok && i < G.members.size(); ++i) ok = c.members[(size_t)at + i] == G.members[i];
        at += (int32_t)G.members.size();
    }
    for (size_t t = 0; ok && t < pixels.size(); ++t) ok = c.feet[t].frame_line == group_of[t];
    expect(ok, "from_pairs: frame lines, members and feet", k);
}

struct LinksCall {
    int rc = 0, rc_count = 0, rc_small = 0;
    int32_t n = -1, n_count = -1;
    std::vector<str_er_line_link> links;
    std::vector<int32_t> line_tracks, members;
    std::vector<str_er_text_track> tracks;
};

LinksCall from_links(const std::vector<uint32_t> &pixels, const std::vector<uint32_t> &frames, const std::vector<Edge> &dups, const std::vector<Edge> &edges,
                     int32_t num, int32_t den)
{
    LinksCall c;
    const int32_t n = (int32_t)pixels.size();
    std::vector<str_er_line_foot> ft;
    for (int32_t t = 0; t < n; ++t) ft.push_back(str_er_line_foot{0, 0, 0, 0, pixels[(size_t)t], -7});
    std::vector<str_er_line_pair> pr;
    for (const Edge &e : dups) pr.push_back(str_er_line_pair{e.a, e.b, e.inter, e.flag});
    std::vector<str_er_line_link> lk;
    for (const Edge &e : edges) lk.push_back(str_er_line_link{e.a, e.b, e.inter, 9u});
    auto feet = block(ft);
    auto pairs = block(pr);
    auto links = block(lk);
    auto fr = block(frames);
    std::unique_ptr<int32_t[]> line_tracks(new int32_t[(size_t)n]), members(new int32_t[(size_t)n]);
    c.rc_count = str_er_text_tracks_from_links(feet.get(), fr.get(), n, pairs.get(), (int32_t)pr.size(), links.get(), (int32_t)lk.size(), num, den, line_tracks.get(),
                                               nullptr, 0, &c.n_count, nullptr);
    if (c.rc_count != STR_ER_OK) { c.rc = c.rc_count; return c; }
    std::unique_ptr<str_er_text_track[]> tracks(new str_er_text_track[(size_t)c.n_count]);
    c.rc = str_er_text_tracks_from_links(feet.get(), fr.get(), n, pairs.get(), (int32_t)pr.size(), links.get(), (int32_t)lk.size(), num, den, line_tracks.get(),
                                         tracks.get(), c.n_count, &c.n, members.get());
    c.links.assign(links.get(), links.get() + lk.size());
    c.line_tracks.assign(line_tracks.get(), line_tracks.get() + n);
    c.members.assign(members.get(), members.get() + n);
    c.tracks.assign(tracks.get(), tracks.get() + c.n_count);
    if (c.n_count > 0) {
        std::unique_ptr<str_er_text_track[]> few(new str_er_text_track[(size_t)c.n_count - 1]);
        int32_t got = -1;
        c.rc_small = str_er_text_tracks_from_links(feet.get(), fr.get(), n, pairs.get(), (int32_t)pr.size(), links.get(), (int32_t)lk.size(), num, den,
                                                   line_tracks.get(), few.get(), c.n_count - 1, &got, members.get());
        if (got != c.n_count) c.rc_small = 1000;
    } else c.rc_small = STR_ER_ECAPACITY;
    return c;
}

// returns the link flags and the track of every line
LinksCall agree_links(const std::vector<uint32_t> &pixels, const std::vector<uint32_t> &frames, const std::vector<Edge> &dups, const std::vector<Edge> &edges,
                      int32_t num, int32_t den, long k)
{
    const LinksCall c = from_links(pixels, frames, dups, edges, num, den);
    std::vector<std::pair<int32_t, int32_t>> joined;
    for (const Edge &e : dups)
        if (e.flag) joined.push_back({e.a, e.b});
    bool ok = c.rc == STR_ER_OK && c.rc_count == STR_ER_OK && c.rc_small == STR_ER_ECAPACITY;
    for (size_t i = 0; ok && i < edges.size(); ++i) {
        const bool link = passes(edges[i].inter, pixels[(size_t)edges[i].a], pixels[(size_t)edges[i].b], num, den);
        ok = c.links[i].link == (link ? 1u : 0u) && c.links[i].a == edges[i].a && c.links[i].b == edges[i].b && c.links[i].inter == edges[i].inter;
        if (link) joined.push_back({edges[i].a, edges[i].b});
    }
    expect(ok, "from_links: codes, counting mode, capacity and link", k);
    if (!ok) return c;
    std::vector<int32_t> group_of;
    const std::vector<Group> groups = partition(pixels, frames, joined, group_of);
    ok = c.n == (int32_t)groups.size() && c.n_count == c.n;
    int32_t at = 0;
    for (size_t g = 0; ok && g < groups.size(); ++g) {
        const Group &G = groups[g];
        const str_er_text_track &T = c.tracks[g];
        ok = T.first_frame == G.key && T.last_frame == G.key1 && T.rep == G.rep && T.pixels == G.pixels && T.first == at && T.count == (int32_t)G.members.size();
        for (size_t i = 0; ok && i < G.members.size(); ++i) ok = c.members[(size_t)at + i] == G.members[i];
        at += (int32_t)G.members.size();
    }
    for (size_t t = 0; ok && t < pixels.size(); ++t) ok = c.line_tracks[t] == group_of[t];
    expect(ok, "from_links: tracks, members and the track of every line", k);
    return c;
}

void check_partitions()
{
    const Box box{0, 0, 10, 10};
    const std::vector<Box> b2(2, box), b3(3, box), b4(4, box);
    // a ~ b ~ c, a and c without a common pixel: one frame line; and with a, c a pair that is no duplicate
    {
        PairsCall c = from_pairs(b3, {100, 100, 100}, {0, 0, 0}, {0, 1, 2}, {{0, 1, 80, 0}, {1, 2, 80, 0}}, 1, 2);
        expect(c.rc == STR_ER_OK && c.n == 1 && c.pairs[0].dup == 1 && c.pairs[1].dup == 1 && c.lines[0].levels == 7 && c.lines[0].rep == 0 && c.lines[0].count == 3 &&
               c.feet[0].frame_line == 0 && c.feet[1].frame_line == 0 && c.feet[2].frame_line == 0, "from_pairs: a chain");
        agree_pairs(b3, {100, 100, 100}, {0, 0, 0}, {0, 1, 2}, {{0, 1, 80, 0}, {1, 2, 80, 0}}, 1, 2, -2);
        c = from_pairs(b3, {100, 100, 100}, {0, 0, 0}, {0, 1, 2}, {{0, 1, 80, 0}, {0, 2, 1, 0}, {1, 2, 80, 0}}, 1, 2);
        expect(c.rc == STR_ER_OK && c.n == 1 && c.pairs[0].dup == 1 && c.pairs[1].dup == 0 && c.pairs[2].dup == 1, "from_pairs: a chain and a pair that is no duplicate");
        // representative: most pixels, ties to the smallest line
        c = from_pairs(b3, {90, 100, 100}, {0, 0, 0}, {3, 3, 4}, {{0, 1, 85, 0}, {1, 2, 95, 0}}, 1, 2);
        expect(c.rc == STR_ER_OK && c.n == 1 && c.lines[0].rep == 1 && c.lines[0].pixels == 100 && c.lines[0].levels == 0x18, "from_pairs: the representative");
        // order: by frame, then by smallest member, whatever the order of the lines' frames
        c = from_pairs(b4, {10, 10, 10, 10}, {1, 0, 1, 0}, {0, 0, 0, 0}, {{0, 2, 10, 0}}, 1, 2);
        expect(c.rc == STR_ER_OK && c.n == 3 && c.lines[0].frame == 0 && c.lines[1].frame == 0 && c.lines[2].frame == 1 && c.feet[0].frame_line == 2 &&
               c.feet[1].frame_line == 0 && c.feet[2].frame_line == 2 && c.feet[3].frame_line == 1, "from_pairs: the order of the frame lines");
        agree_pairs(b4, {10, 10, 10, 10}, {1, 0, 1, 0}, {0, 0, 0, 0}, {{0, 2, 10, 0}}, 1, 2, -3);
        // 64-bit products: 2^31 pixels at den = 65535
        c = from_pairs(b2, {1u << 31, 1u << 31}, {0, 0}, {0, 0}, {{0, 1, 1u << 31, 0}}, 65535, 65535);
        expect(c.rc == STR_ER_OK && c.pairs[0].dup == 1, "from_pairs: 2^31 pixels");
        // errors
        const std::vector<Edge> wrong = {{0, 1, 5, 0}, {1, 1, 5, 0}, {2, 1, 5, 0}, {0, 4, 5, 0}, {-1, 2, 5, 0}, {0, 2, 0, 0}, {0, 2, 11, 0}};
        for (const Edge &e : wrong) expect(from_pairs(b4, {10, 10, 10, 10}, {1, 0, 1, 0}, {0, 0, 0, 0}, {e}, 1, 2).rc == STR_ER_EINVAL, "from_pairs: a pair refused", e.a * 10 + e.b);
        expect(from_pairs({box}, {10}, {0}, {0}, {}, 0, 1).rc == STR_ER_EINVAL && from_pairs({box}, {10}, {0}, {0}, {}, 2, 1).rc == STR_ER_EINVAL &&
               from_pairs({box}, {10}, {0}, {0}, {}, 1, 65536).rc == STR_ER_EINVAL, "from_pairs: num / den refused");
        c = from_pairs({}, {}, {}, {}, {}, 1, 2);
        expect(c.rc == STR_ER_OK && c.n == 0, "from_pairs: no line at all");
    }
    // a chain over 40 frames, one line a frame: one track; cut in the middle by an overlap that is no link: two
    {
        const int32_t n = 40;
        std::vector<uint32_t> px((size_t)n, 100), fr;
        std::vector<Edge> chain, cut;
        for (int32_t t = 0; t < n; ++t) fr.push_back((uint32_t)t);
        for (int32_t t = 0; t + 1 < n; ++t) { chain.push_back({t, t + 1, 80, 0}); cut.push_back({t, t + 1, t != 19 ? 80u : 10u, 0}); }
        LinksCall c = agree_links(px, fr, {}, chain, 1, 2, -4);
        expect(c.n == 1 && c.tracks[0].first_frame == 0 && c.tracks[0].last_frame == 39 && c.tracks[0].first == 0 && c.tracks[0].count == n && c.tracks[0].rep == 0 &&
               c.tracks[0].pixels == 100, "from_links: a chain");
        c = agree_links(px, fr, {}, cut, 1, 2, -5);
        expect(c.n == 2 && c.line_tracks[19] == 0 && c.line_tracks[20] == 1 && c.tracks[1].first_frame == 20 && c.links[19].link == 0, "from_links: a chain cut");
        // a track that splits and rejoins; two halves joined only through a duplicate pair within the frame
        c = agree_links({100, 50, 50, 100}, {0, 1, 1, 2}, {}, {{0, 1, 50, 0}, {0, 2, 50, 0}, {1, 3, 50, 0}, {2, 3, 50, 0}}, 1, 3, -6);
        expect(c.n == 1 && c.tracks[0].count == 4 && c.tracks[0].rep == 0, "from_links: split and rejoined");
        c = agree_links({100, 100, 100, 100, 100}, {0, 0, 1, 1, 2}, {{0, 1, 1, 1}}, {{0, 2, 90, 0}, {1, 3, 90, 0}, {3, 4, 90, 0}}, 1, 2, -7);
        expect(c.n == 1, "from_links: joined through a duplicate");
        c = agree_links({100, 100, 100, 100, 100}, {0, 0, 1, 1, 2}, {{0, 1, 1, 0}}, {{0, 2, 90, 0}, {1, 3, 90, 0}, {3, 4, 90, 0}}, 1, 2, -8);
        expect(c.n == 2 && c.line_tracks == std::vector<int32_t>({0, 1, 0, 1, 1}), "from_links: a pair that is no duplicate joins nothing");
        c = agree_links({1u << 31, 1u << 31}, {0, 1}, {}, {{0, 1, 1u << 31, 0}}, 65535, 65535, -9);
        expect(c.links[0].link == 1, "from_links: 2^31 pixels");
        c = agree_links({1u << 31, 1u << 31}, {0, 1}, {}, {{0, 1, (1u << 31) - 1, 0}}, 65535, 65535, -10);
        expect(c.links[0].link == 0, "from_links: 2^31 pixels, one less in common");
        // representative and order, whatever the order of the lines
        c = agree_links({90, 100, 100, 10}, {2, 1, 0, 0}, {}, {{2, 1, 90, 0}, {1, 0, 85, 0}}, 1, 2, -11);
        expect(c.n == 2 && c.tracks[0].rep == 1 && c.tracks[0].pixels == 100 && c.line_tracks == std::vector<int32_t>({0, 0, 0, 1}) && c.tracks[1].first_frame == 0,
               "from_links: the representative and the order");
        c = agree_links({5, 6, 7}, {1, 0, 1}, {}, {}, 1, 2, -12);
        expect(c.n == 3 && c.line_tracks == std::vector<int32_t>({1, 0, 2}), "from_links: lines without a pair or a link");
        // errors
        const std::vector<uint32_t> p4 = {10, 10, 10, 10}, f4 = {0, 1, 1, 3};
        const std::vector<Edge> wrong = {{0, 3, 5, 0}, {1, 0, 5, 0}, {1, 2, 5, 0}, {0, 4, 5, 0}, {-1, 1, 5, 0}, {0, 1, 0, 0}, {0, 1, 11, 0}, {2, 3, 5, 0}};
        for (const Edge &e : wrong) expect(from_links(p4, f4, {}, {e}, 1, 2).rc == STR_ER_EINVAL, "from_links: a link refused", e.a * 10 + e.b);
        const std::vector<Edge> wrong_pairs = {{0, 1, 1, 1}, {2, 1, 1, 1}, {1, 1, 1, 1}, {1, 4, 1, 1}};
        for (const Edge &e : wrong_pairs) expect(from_links(p4, f4, {e}, {}, 1, 2).rc == STR_ER_EINVAL, "from_links: a pair refused", e.a * 10 + e.b);
        expect(from_links({10}, {0}, {}, {}, 0, 1).rc == STR_ER_EINVAL && from_links({10}, {0}, {}, {}, 2, 1).rc == STR_ER_EINVAL &&
               from_links({10}, {0}, {}, {}, 1, 65536).rc == STR_ER_EINVAL, "from_links: num / den refused");
        expect(from_links({}, {}, {}, {}, 1, 2).rc == STR_ER_OK && from_links({}, {}, {}, {}, 1, 2).n == 0, "from_links: no line at all");
    }
    // the boundary: inter * den == num * union passes, one pixel less does not
    const int32_t nd[5][2] = {{1, 2}, {1, 3}, {2, 3}, {1, 1}, {7, 50}};
    for (const auto &q : nd) {
        const int32_t num = q[0], den = q[1];
        const uint32_t sizes[3][2] = {{300, 300}, {150, 450}, {1000, 50u * (uint32_t)den}};
        for (const auto &sz : sizes)
            for (uint32_t k = 1; k <= std::min(sz[0], sz[1]); ++k) {
                const bool exact = (uint64_t)k * (uint64_t)den == (uint64_t)num * (sz[0] + sz[1] - k);
                if (!exact && (uint64_t)(k + 1) * (uint64_t)den != (uint64_t)num * (sz[0] + sz[1] - k - 1)) continue;
                const PairsCall c = from_pairs(b2, {sz[0], sz[1]}, {0, 0}, {0, 0}, {{0, 1, k, 0}}, num, den);
                expect(c.rc == STR_ER_OK && c.pairs[0].dup == (exact ? 1u : 0u) && c.n == (exact ? 1 : 2), "from_pairs: the boundary", (long)k);
                const LinksCall l = from_links({sz[0], sz[1]}, {0, 1}, {}, {{0, 1, k, 0}}, num, den);
                expect(l.rc == STR_ER_OK && l.links[0].link == (exact ? 1u : 0u) && l.n == (exact ? 1 : 2), "from_links: the boundary", (long)k);
            }
    }
    // random small cases: at most 12 lines and 4 frames
    const int32_t thr[6][2] = {{1, 2}, {1, 1}, {1, 50}, {3, 4}, {65535, 65535}, {1, 65535}};
    const uint32_t sizes[8] = {0, 1, 7, 50, 50, 200, 4000, 1u << 31};
    for (long k = 0; k < 3000; ++k) {
        const int32_t n = below(13), n_frames = 1 + below(4);
        std::vector<uint32_t> pixels, frames;
        std::vector<uint8_t> pyr;
        std::vector<Box> boxes;
        for (int32_t t = 0; t < n; ++t) {
            pixels.push_back(sizes[below(8)]);
            frames.push_back((uint32_t)below((uint32_t)n_frames));
            pyr.push_back((uint8_t)below(k % 7 ? 8 : 40));
            boxes.push_back(pixels.back() ? Box{below(1900), below(1000), 1 + below(300), 1 + below(80)} : Box{0, 0, 0, 0});
        }
        if (k % 3) std::sort(frames.begin(), frames.end());
        std::vector<Edge> pairs, dups, links;
        for (int32_t a = 0; a < n; ++a)
            for (int32_t b = 0; b < n; ++b) {
                const uint32_t m = std::min(pixels[(size_t)a], pixels[(size_t)b]);
                if (m == 0) continue;
                const uint32_t choice[4] = {1, std::max(1u, m / 2), std::max(1u, m - 1), m};
                if (a < b && frames[(size_t)a] == frames[(size_t)b] && below(4) == 0) {
                    pairs.push_back({a, b, choice[below(4)], 0});
                    dups.push_back({a, b, 1, (uint32_t)below(2)});
                }
                if (frames[(size_t)b] == frames[(size_t)a] + 1 && below(5) == 0) links.push_back({a, b, choice[below(4)], 0});
            }
        agree_pairs(boxes, pixels, frames, pyr, pairs, thr[k % 6][0], thr[k % 6][1], k);
        agree_links(pixels, frames, dups, links, thr[k % 6][0], thr[k % 6][1], k);
    }
}

// ---- the hulls and the boxes -------------------------------------------------------------------------------------------------------------

// O(n^3): p -> q is a hull edge iff every other point lies strictly to its clockwise side or on the segment between them
std::vector<Pt> brute_hull(std::vector<Pt> p)
{
    std::sort(p.begin(), p.end(), before);
    p.erase(std::unique(p.begin(), p.end()), p.end());
    bool line = true;
    for (size_t i = 2; i < p.size(); ++i) line = line && cross(p[0], p[1], p[i]) == 0;
    if (p.size() <= 2) return p;
    if (line) return {p.front(), p.back()};
    std::vector<int32_t> next(p.size(), -1);
    for (size_t a = 0; a < p.size(); ++a)
        for (size_t b = 0; b < p.size(); ++b) {
            if (a == b) continue;
            bool edge = true;
            for (size_t r = 0; edge && r < p.size(); ++r) {
                if (r == a || r == b) continue;
                const i128 t = cross(p[a], p[b], p[r]);
                const bool between = std::min(p[a].x, p[b].x) <= p[r].x && p[r].x <= std::max(p[a].x, p[b].x) && std::min(p[a].y, p[b].y) <= p[r].y &&
                                     p[r].y <= std::max(p[a].y, p[b].y);
                edge = t > 0 || (t == 0 && between);
            }
            if (edge) next[a] = (int32_t)b;
        }
    std::vector<Pt> hull;
    for (int32_t at = 0; hull.size() <= p.size(); at = next[(size_t)at]) {          // (p[0] is the smallest (y, x): a vertex)
        if (at < 0 || (at == 0 && !hull.empty())) break;
        hull.push_back(p[(size_t)at]);
    }
    return hull;
}

void check_hull(const std::vector<Pt> &pts, long k)
{
    std::vector<int32_t> xy;
    for (const Pt &p : pts) { xy.push_back(p.x); xy.push_back(p.y); }
    auto in = block(xy);
    const std::vector<Pt> ref = brute_hull(pts);
    int32_t n_count = -1, n = -1;
    const int rc_count = str_er_hull_of_points(in.get(), (int32_t)pts.size(), nullptr, 0, &n_count);
    std::unique_ptr<int32_t[]> out(new int32_t[2 * ref.size()]);
    const int rc = str_er_hull_of_points(in.get(), (int32_t)pts.size(), out.get(), (int32_t)ref.size(), &n);
    bool ok = rc_count == STR_ER_OK && rc == STR_ER_OK && n_count == (int32_t)ref.size() && n == n_count;
    for (size_t i = 0; ok && i < ref.size(); ++i) ok = out[2 * i] == ref[i].x && out[2 * i + 1] == ref[i].y;
    if (!ref.empty()) {
        std::unique_ptr<int32_t[]> few(new int32_t[2 * (ref.size() - 1)]);
        int32_t got = -1;
        ok = ok && str_er_hull_of_points(in.get(), (int32_t)pts.size(), few.get(), (int32_t)ref.size() - 1, &got) == STR_ER_ECAPACITY && got == (int32_t)ref.size();
    }
    expect(ok, "hull_of_points against the brute-force hull", k);
    str_er_line_geom G{};
    if (ref.size() < 3) {
        if (!ref.empty()) expect(str_er_quad_from_hull(out.get(), (int32_t)ref.size(), &G) == STR_ER_EINVAL, "quad_from_hull: fewer than three vertices", k);
        return;
    }
    bool in_range = true;
    for (const Pt &p : ref) in_range = in_range && p.x >= 0 && p.x <= 65535 && p.y >= 0 && p.y <= 65535;
    if (!in_range) return;
    // O(n^2): the box of every edge over all vertices, the areas compared as exact fractions, ties to the smallest edge
    const int32_t m = (int32_t)ref.size();
    int32_t best = -1;
    int64_t b_ex = 0, b_ey = 0, b_d0 = 0, b_d1 = 0, b_c0 = 0, b_c1 = 0, b_den = 1;
    i128 b_num = 0, area2 = 0;
    for (int32_t i = 0; i < m; ++i) {
        const Pt &p = ref[(size_t)i], &q = ref[(size_t)((i + 1) % m)];
        area2 += (i128)p.x * q.y - (i128)q.x * p.y;
        const int64_t ex = (int64_t)q.x - p.x, ey = (int64_t)q.y - p.y;
        int64_t d0 = 0, d1 = 0, c0 = 0, c1 = 0;
        for (int32_t j = 0; j < m; ++j) {
            const int64_t d = ref[(size_t)j].x * ex + ref[(size_t)j].y * ey, c = -ref[(size_t)j].x * ey + ref[(size_t)j].y * ex;
            d0 = j ? std::min(d0, d) : d; d1 = j ? std::max(d1, d) : d; c0 = j ? std::min(c0, c) : c; c1 = j ? std::max(c1, c) : c;
        }
        const int64_t den = ex * ex + ey * ey;
        const i128 num = (i128)(d1 - d0) * (c1 - c0);
        if (best < 0 || num * b_den < b_num * den) { best = i; b_ex = ex; b_ey = ey; b_d0 = d0; b_d1 = d1; b_c0 = c0; b_c1 = c1; b_num = num; b_den = den; }
    }
    ok = str_er_quad_from_hull(out.get(), m, &G) == STR_ER_OK && G.hull_area2 == (uint64_t)area2 && G.edge == best && G.ex == b_ex && G.ey == b_ey && G.dmin == b_d0 &&
         G.dmax == b_d1 && G.cmin == b_c0 && G.cmax == b_c1;
    const int64_t dd[4] = {b_d0, b_d1, b_d1, b_d0}, cs[4] = {b_c0, b_c0, b_c1, b_c1};
    for (int q = 0; ok && q < 4; ++q)
        ok = G.qx[q] == (double)(dd[q] * b_ex - cs[q] * b_ey) / (double)b_den && G.qy[q] == (double)(dd[q] * b_ey + cs[q] * b_ex) / (double)b_den;
    expect(ok, "quad_from_hull against the brute-force box", k);
}

void check_hulls()
{
    // the degenerate sets
    check_hull({}, -1);
    check_hull({{5, 7}}, -2);
    check_hull({{5, 7}, {5, 7}, {5, 7}}, -3);
    check_hull({{9, 1}, {2, 3}}, -4);
    check_hull({{0, 0}, {3, 3}, {1, 1}, {2, 2}, {3, 3}}, -5);
    check_hull({{4, 9}, {4, 2}, {4, 5}}, -6);
    check_hull({{7, 3}, {1, 3}, {4, 3}, {4, 3}}, -7);
    check_hull({{0, 0}, {1, 0}, {1, 1}, {0, 1}}, -8);
    check_hull({{0, 0}, {2, 0}, {1, 0}, {2, 2}, {0, 2}, {1, 1}, {2, 1}, {0, 0}}, -9);
    // the corners of the coordinate range: the largest products
    check_hull({{0, 0}, {65535, 0}, {65535, 65535}, {0, 65535}}, -10);
    check_hull({{0, 0}, {65535, 65535}, {65535, 0}}, -11);
    check_hull({{0, 65535}, {65535, 0}, {0, 0}, {65535, 65534}, {1, 65535}}, -12);
    check_hull({{0, 1}, {65534, 0}, {65535, 65534}, {1, 65535}}, -13);
    check_hull({{-5, 3}, {2147483647, 0}, {-2147483647 - 1, 2147483647}, {0, -2147483647 - 1}}, -14);          // (the hull alone: the box needs [0, 65535])
    // what quad_from_hull refuses
    {
        str_er_line_geom G{};
        const std::vector<std::vector<int32_t>> wrong = {{0, 0, 1, 0},                            // two vertices
                                                          {0, 0, 0, 1, 1, 1, 1, 0},                // counter-clockwise
                                                          {1, 0, 1, 1, 0, 1, 0, 0},                // not from the smallest (y, x)
                                                          {0, 0, 1, 0, 2, 0, 2, 2},                // a collinear vertex
                                                          {0, 0, 65536, 0, 65536, 1},              // outside the range
                                                          {0, 0, -1, 0, 0, 1},
                                                          {0, 0, 2, 0, 2, 2, 0, 0, 2, 0, 2, 2}};   // twice round
        for (size_t i = 0; i < wrong.size(); ++i) {
            auto v = block(wrong[i]);
            expect(str_er_quad_from_hull(v.get(), (int32_t)(wrong[i].size() / 2), &G) == STR_ER_EINVAL, "quad_from_hull: refused", (long)i);
        }
        int32_t n = 0;
        expect(str_er_quad_from_hull(nullptr, 3, &G) == STR_ER_EINVAL && str_er_hull_of_points(nullptr, 1, nullptr, 0, &n) == STR_ER_EINVAL &&
               str_er_hull_of_points(nullptr, 0, nullptr, 0, nullptr) == STR_ER_EINVAL && str_er_hull_of_points(nullptr, -1, nullptr, 0, &n) == STR_ER_EINVAL,
               "missing arguments");
    }
    // random sets of at most 64 points: on small grids (duplicates, collinear runs), over the whole range, and on its border
    for (long k = 0; k < 1500; ++k) {
        const int32_t n = below(65);
        const uint32_t span = k % 4 == 0 ? 4 : k % 4 == 1 ? 12 : k % 4 == 2 ? 300 : 65536;
        const int32_t  base = k % 8 >= 4 && span < 65536 ? (int32_t)(65536 - span) : 0;
        std::vector<Pt> pts;
        for (int32_t i = 0; i < n; ++i) {
            Pt p{base + below(span), base + below(span)};
            if (span == 65536 && k % 5 == 0) (below(2) ? p.x : p.y) = below(2) ? 0 : 65535;
            pts.push_back(p);
        }
        check_hull(pts, k);
    }
}

} // namespace

int main()
{
    check_partitions();
    check_hulls();
    printf("%ld checked, %ld wrong\n", cases, bad);
    return bad ? 1 : 0;
}
