// lines_host.cpp -- the C ABI, part 8a: the host side of the line stage that touches no device.  The frame lines of a call from the
// pairs of its lines (str_er_frame_lines_from_pairs; the contract is at str_er_line_foot in str_er.h), its text tracks from the links
// (str_er_text_tracks_from_links; str_er_line_link), the convex hull of points and the oriented box of a hull (str_er_hull_of_points,
// str_er_quad_from_hull; str_er_line_geom), the ratio test of duplicates and links (overlap_passes) and the geometry of the frame
// lines from that of their members (frame_line_geoms).  Pure host and HIP-free, as words_host.cpp is: it includes nothing of the
// library but the public header, so that tests/cpp/lines_host_check.cpp links this file alone under the host sanitizers.  The detect
// calls, str_er_line_feet_regions, str_er_link_feet and str_er_feet_geom (api_frame_lines.cpp) use these same functions.
#include "../../include/str_er.h"

#include <algorithm>
#include <array>
#include <numeric>
#include <vector>

namespace str_er_host {

// inter * den >= num * (pa + pb - inter): the two footprints of pa and pb pixels, inter of them common, are duplicates (links) at
// num / den.  inter <= min(pa, pb) < 2^32 and num <= den <= 65535: both sides stay below 2^49.
bool overlap_passes(uint32_t inter, uint32_t pa, uint32_t pb, int32_t num, int32_t den)
{
    return (uint64_t)inter * (uint64_t)den >= (uint64_t)num * ((uint64_t)pa + (uint64_t)pb - (uint64_t)inter);
}

// the geometry of frame lines: the hull of the union of the members' hull vertices (appended to points, which holds the members'
// vertices), the moments of the representative.  Not STR_ER_OK: a hull failed (the members' geometry is no geometry)
int frame_line_geoms(const str_er_frame_line *frame_lines, size_t n_frame_lines, const int32_t *members, const str_er_line_geom *line_geoms,
                     std::vector<int32_t> &points, std::vector<str_er_line_geom> &out)
{
    out.assign(n_frame_lines, str_er_line_geom{});
    std::vector<int32_t> uni, hull;
    for (size_t i = 0; i < n_frame_lines; ++i) {
        const str_er_frame_line &FL = frame_lines[i];
        str_er_line_geom &G = out[i];
        G.edge = -1;
        uni.clear();
        for (int32_t k = FL.first; k < FL.first + FL.count; ++k) {
            const str_er_line_geom &M = line_geoms[(size_t)members[(size_t)k]];
            uni.insert(uni.end(), points.begin() + 2 * (size_t)M.first, points.begin() + 2 * ((size_t)M.first + M.count));
        }
        if (FL.rep >= 0) {
            const str_er_line_geom &M = line_geoms[(size_t)FL.rep];
            G.pixels = M.pixels; G.m10 = M.m10; G.m01 = M.m01; G.m20 = M.m20; G.m11 = M.m11; G.m02 = M.m02;
        }
        if (uni.empty()) continue;
        if (FL.count == 1) {            // (one member: its hull and its box)
            G = line_geoms[(size_t)members[(size_t)FL.first]];
            G.first = (uint32_t)(points.size() / 2);
            points.insert(points.end(), uni.begin(), uni.end());
            continue;
        }
        hull.resize(uni.size());
        int32_t nh = 0;
        int rc = str_er_hull_of_points(uni.data(), (int32_t)(uni.size() / 2), hull.data(), (int32_t)(uni.size() / 2), &nh);
        if (rc != STR_ER_OK || (rc = str_er_quad_from_hull(hull.data(), nh, &G)) != STR_ER_OK) return rc;
        G.first = (uint32_t)(points.size() / 2); G.count = (uint32_t)nh;
        points.insert(points.end(), hull.begin(), hull.begin() + 2 * (size_t)nh);
    }
    return STR_ER_OK;
}

} // namespace str_er_host

namespace {

using str_er_host::overlap_passes;
using i128 = __int128;

// > 0: o -> a -> b turns clockwise on screen (x to the right, y down)
inline i128 turn(const int32_t *o, const int32_t *a, const int32_t *b)
{
    return (i128)((int64_t)a[0] - o[0]) * ((int64_t)b[1] - o[1]) - (i128)((int64_t)a[1] - o[1]) * ((int64_t)b[0] - o[0]);
}

int find_root(std::vector<int32_t> &parent, int32_t t)
{
    while (parent[(size_t)t] != t) { parent[(size_t)t] = parent[(size_t)parent[(size_t)t]]; t = parent[(size_t)t]; }
    return t;
}

// the root of a component is its smallest line
void join(std::vector<int32_t> &parent, int32_t a, int32_t b)
{
    const int32_t ra = find_root(parent, a), rb = find_root(parent, b);
    if (ra != rb) parent[(size_t)std::max(ra, rb)] = std::min(ra, rb);
}

// a record's common pixels: some, and no more than either footprint has
bool inter_ok(uint32_t inter, const str_er_line_foot *feet, int32_t a, int32_t b) { return inter != 0 && inter <= feet[a].pixels && inter <= feet[b].pixels; }

// a list of pairs of lines of one frame, a < b, as both functions take it
bool pairs_ok(const str_er_line_foot *feet, const uint32_t *frames_of_lines, int32_t n_lines, const str_er_line_pair *pairs, int32_t n_pairs)
{
    for (int32_t k = 0; k < n_pairs; ++k) {
        const str_er_line_pair &P = pairs[k];
        if (P.a < 0 || P.a >= P.b || P.b >= n_lines || frames_of_lines[P.a] != frames_of_lines[P.b]) return false;
        if (!inter_ok(P.inter, feet, P.a, P.b)) return false;
    }
    return true;
}

// The components of `parent` as groups (G: str_er_frame_line or str_er_text_track), ordered by the key of their root, then by the root
// (their smallest member).  group_of[t]: the group of line t; *n_groups: their number -- both set whatever else happens.  With
// groups: head(G, root) fills what is the group's own in a zeroed record, then first / count / members (ascending) and the
// representative: the member with the most pixels, a tie stays with the smaller line.  STR_ER_ECAPACITY: more groups than cap.
template <typename G, typename Head>
int group_by_root(std::vector<int32_t> &parent, const uint32_t *key, const str_er_line_foot *feet, std::vector<int32_t> &group_of, G *groups, int32_t cap,
                  int32_t *n_groups, int32_t *members, Head head)
{
    const int32_t n_lines = (int32_t)parent.size();
    std::vector<int32_t> roots;
    for (int32_t t = 0; t < n_lines; ++t)
        if (find_root(parent, t) == t) roots.push_back(t);
    std::sort(roots.begin(), roots.end(), [&](int32_t p, int32_t q) { return key[p] != key[q] ? key[p] < key[q] : p < q; });
    std::vector<int32_t> index_of((size_t)n_lines, -1);
    for (size_t i = 0; i < roots.size(); ++i) index_of[(size_t)roots[i]] = (int32_t)i;
    group_of.resize((size_t)n_lines);
    for (int32_t t = 0; t < n_lines; ++t) group_of[(size_t)t] = index_of[(size_t)find_root(parent, t)];
    *n_groups = (int32_t)roots.size();
    if (!groups) return STR_ER_OK;
    if ((int32_t)roots.size() > cap) return STR_ER_ECAPACITY;
    for (size_t i = 0; i < roots.size(); ++i) {
        groups[i] = G{};
        groups[i].rep = -1;
        head(groups[i], roots[i]);
    }
    for (int32_t t = 0; t < n_lines; ++t) ++groups[group_of[(size_t)t]].count;
    int32_t at = 0;
    for (size_t i = 0; i < roots.size(); ++i) { groups[i].first = at; at += groups[i].count; groups[i].count = 0; }
    for (int32_t t = 0; t < n_lines; ++t) {          // (ascending t: the members ascend, and a tie of pixels stays with the smaller line)
        G &g = groups[group_of[(size_t)t]];
        members[g.first + g.count++] = t;
        if (g.rep < 0 || feet[t].pixels > g.pixels) { g.rep = t; g.pixels = feet[t].pixels; }
    }
    return STR_ER_OK;
}

} // namespace

extern "C" {

int str_er_frame_lines_from_pairs(str_er_line_foot *feet, const uint32_t *frames_of_lines, const uint8_t *pyr_of_lines, int32_t n_lines,
                                  str_er_line_pair *pairs, int32_t n_pairs, int32_t num, int32_t den, str_er_frame_line *frame_lines,
                                  int32_t cap_frame_lines, int32_t *n_frame_lines, int32_t *members)
try {
    if (n_lines < 0 || n_pairs < 0 || !n_frame_lines || num < 1 || num > den || den > 65535) return STR_ER_EINVAL;
    if (n_lines > 0 && (!feet || !frames_of_lines || !pyr_of_lines)) return STR_ER_EINVAL;
    if ((n_pairs > 0 && !pairs) || (frame_lines && n_lines > 0 && !members) || (frame_lines && cap_frame_lines < 0)) return STR_ER_EINVAL;
    if (!pairs_ok(feet, frames_of_lines, n_lines, pairs, n_pairs)) return STR_ER_EINVAL;
    // the duplicates joined
    std::vector<int32_t> parent((size_t)n_lines);
    std::iota(parent.begin(), parent.end(), 0);
    for (int32_t k = 0; k < n_pairs; ++k) {
        str_er_line_pair &P = pairs[k];
        P.dup = overlap_passes(P.inter, feet[P.a].pixels, feet[P.b].pixels, num, den) ? 1u : 0u;
        if (P.dup) join(parent, P.a, P.b);
    }
    // the frame lines: by frame, then by smallest member
    std::vector<int32_t> group_of;
    const int rc = group_by_root(parent, frames_of_lines, feet, group_of, frame_lines, cap_frame_lines, n_frame_lines, members,
                                 [&](str_er_frame_line &G, int32_t root) { G.frame = frames_of_lines[root]; });
    for (int32_t t = 0; t < n_lines; ++t) feet[t].frame_line = group_of[(size_t)t];
    if (rc != STR_ER_OK || !frame_lines) return rc;
    for (int32_t t = 0; t < n_lines; ++t) {          // on top: the levels of the members and the union of their foot boxes
        str_er_frame_line      &G = frame_lines[feet[t].frame_line];
        const str_er_line_foot &F = feet[t];
        if (pyr_of_lines[t] < 32) G.levels |= 1u << pyr_of_lines[t];
        if (F.w > 0 && F.h > 0) {
            if (G.w == 0) { G.x = F.x; G.y = F.y; G.w = F.w; G.h = F.h; }
            else {
                const int32_t x1 = std::max(G.x + G.w, F.x + F.w), y1 = std::max(G.y + G.h, F.y + F.h);
                G.x = std::min(G.x, F.x); G.y = std::min(G.y, F.y); G.w = x1 - G.x; G.h = y1 - G.y;
            }
        }
    }
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

int str_er_text_tracks_from_links(const str_er_line_foot *feet, const uint32_t *frames_of_lines, int32_t n_lines, const str_er_line_pair *pairs,
                                  int32_t n_pairs, str_er_line_link *links, int32_t n_links, int32_t num, int32_t den, int32_t *line_tracks,
                                  str_er_text_track *tracks, int32_t cap_tracks, int32_t *n_tracks, int32_t *members)
try {
    if (n_lines < 0 || n_pairs < 0 || n_links < 0 || !n_tracks || num < 1 || num > den || den > 65535) return STR_ER_EINVAL;
    if (n_lines > 0 && (!feet || !frames_of_lines || !line_tracks)) return STR_ER_EINVAL;
    if ((n_pairs > 0 && !pairs) || (n_links > 0 && !links) || (tracks && n_lines > 0 && !members) || (tracks && cap_tracks < 0)) return STR_ER_EINVAL;
    if (!pairs_ok(feet, frames_of_lines, n_lines, pairs, n_pairs)) return STR_ER_EINVAL;
    for (int32_t k = 0; k < n_links; ++k) {
        const str_er_line_link &P = links[k];
        if (P.a < 0 || P.a >= n_lines || P.b < 0 || P.b >= n_lines) return STR_ER_EINVAL;
        if ((uint64_t)frames_of_lines[P.b] != (uint64_t)frames_of_lines[P.a] + 1u) return STR_ER_EINVAL;
        if (!inter_ok(P.inter, feet, P.a, P.b)) return STR_ER_EINVAL;
    }
    // duplicates and links joined
    std::vector<int32_t> parent((size_t)n_lines);
    std::iota(parent.begin(), parent.end(), 0);
    for (int32_t k = 0; k < n_pairs; ++k)
        if (pairs[k].dup) join(parent, pairs[k].a, pairs[k].b);
    for (int32_t k = 0; k < n_links; ++k) {
        str_er_line_link &P = links[k];
        P.link = overlap_passes(P.inter, feet[P.a].pixels, feet[P.b].pixels, num, den) ? 1u : 0u;
        if (P.link) join(parent, P.a, P.b);
    }
    // the tracks: by first frame, then by smallest member
    std::vector<uint32_t> f0((size_t)n_lines, UINT32_MAX), f1((size_t)n_lines, 0);
    for (int32_t t = 0; t < n_lines; ++t) {
        const size_t q = (size_t)find_root(parent, t);
        f0[q] = std::min(f0[q], frames_of_lines[t]); f1[q] = std::max(f1[q], frames_of_lines[t]);
    }
    std::vector<int32_t> group_of;
    const int rc = group_by_root(parent, f0.data(), feet, group_of, tracks, cap_tracks, n_tracks, members,
                                 [&](str_er_text_track &G, int32_t root) { G.first_frame = f0[(size_t)root]; G.last_frame = f1[(size_t)root]; });
    for (int32_t t = 0; t < n_lines; ++t) line_tracks[t] = group_of[(size_t)t];
    return rc;
} catch (...) { return STR_ER_ENOMEM; }

int str_er_hull_of_points(const int32_t *xy, int32_t n, int32_t *out_xy, int32_t cap, int32_t *n_out)
try {
    if (n < 0 || !n_out || (n > 0 && !xy) || (out_xy && cap < 0)) return STR_ER_EINVAL;
    // Andrew's monotone chain over the points sorted by (y, x): down the right side, then up the left side, every turn strictly clockwise
    std::vector<std::array<int32_t, 2>> p((size_t)n);
    for (int32_t i = 0; i < n; ++i) p[(size_t)i] = {xy[2 * i], xy[2 * i + 1]};
    std::sort(p.begin(), p.end(), [](const std::array<int32_t, 2> &a, const std::array<int32_t, 2> &b) { return a[1] != b[1] ? a[1] < b[1] : a[0] < b[0]; });
    p.erase(std::unique(p.begin(), p.end()), p.end());
    std::vector<std::array<int32_t, 2>> st;
    if (p.size() <= 2) st = p;
    else {
        st.reserve(2 * p.size());
        for (size_t i = 0; i < p.size(); ++i) {
            while (st.size() >= 2 && turn(st[st.size() - 2].data(), st.back().data(), p[i].data()) <= 0) st.pop_back();
            st.push_back(p[i]);
        }
        const size_t low = st.size() + 1;
        for (size_t i = p.size() - 1; i-- > 0;) {
            while (st.size() >= low && turn(st[st.size() - 2].data(), st.back().data(), p[i].data()) <= 0) st.pop_back();
            st.push_back(p[i]);
        }
        st.pop_back();
    }
    *n_out = (int32_t)st.size();
    if (!out_xy) return STR_ER_OK;
    if ((int32_t)st.size() > cap) return STR_ER_ECAPACITY;
    for (size_t i = 0; i < st.size(); ++i) { out_xy[2 * i] = st[i][0]; out_xy[2 * i + 1] = st[i][1]; }
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

int str_er_quad_from_hull(const int32_t *xy, int32_t n, str_er_line_geom *out)
try {
    if (!xy || !out || n < 3) return STR_ER_EINVAL;
    for (int32_t i = 0; i < 2 * n; ++i)
        if (xy[i] < 0 || xy[i] > 65535) return STR_ER_EINVAL;
    // a hull in the stated order: it starts at the smallest (y, x), every turn is strictly clockwise, and it goes round once (y falls
    // only after it has risen, and then never rises again)
    int32_t flips = 0;
    int     first_sign = 0, last_sign = 0;         // of the y steps that are not level
    for (int32_t i = 0; i < n; ++i) {
        const int32_t *p = xy + 2 * (size_t)i, *q = xy + 2 * (size_t)((i + 1) % n), *w = xy + 2 * (size_t)((i + 2) % n);
        if (i > 0 && (p[1] < xy[1] || (p[1] == xy[1] && p[0] <= xy[0]))) return STR_ER_EINVAL;
        if (turn(p, q, w) <= 0) return STR_ER_EINVAL;
        const int sg = (q[1] > p[1]) - (q[1] < p[1]);
        if (sg == 0) continue;
        if (last_sign != 0 && sg != last_sign) ++flips;
        if (first_sign == 0) first_sign = sg;
        last_sign = sg;
    }
    if (flips + (first_sign != last_sign ? 1 : 0) != 2) return STR_ER_EINVAL;
    const auto V = [&](int32_t k) { return xy + 2 * (size_t)(k % n); };
    i128 area2 = 0;
    for (int32_t i = 0; i < n; ++i) area2 += (i128)V(i)[0] * V(i + 1)[1] - (i128)V(i + 1)[0] * V(i)[1];
    // rotating calipers: for the edge i the vertices with the largest d, the largest c and the smallest d only move forward as i does
    // (c is smallest on the edge itself: the hull lies on the side of its normal); every value is exact in 64 bits
    int32_t pd = 0, pc = 0, pm = 0;         // (positions, taken modulo n)
    int32_t best = -1;
    int64_t b_ex = 0, b_ey = 0, b_d0 = 0, b_d1 = 0, b_c0 = 0, b_c1 = 0;
    i128    b_num = 0;
    int64_t b_den = 1;
    for (int32_t i = 0; i < n; ++i) {
        const int64_t ex = (int64_t)V(i + 1)[0] - V(i)[0], ey = (int64_t)V(i + 1)[1] - V(i)[1];
        const auto d = [&](int32_t k) { return V(k)[0] * ex + V(k)[1] * ey; };
        const auto cc = [&](int32_t k) { return -V(k)[0] * ey + V(k)[1] * ex; };
        if (i == 0) {
            for (int32_t k = 1; k < n; ++k) {
                if (d(k) > d(pd)) pd = k;
                if (cc(k) > cc(pc)) pc = k;
                if (d(k) < d(pm)) pm = k;
            }
        } else {
            for (int32_t g = 0; g < n && d(pd + 1) > d(pd); ++g) pd = (pd + 1) % n;
            for (int32_t g = 0; g < n && cc(pc + 1) > cc(pc); ++g) pc = (pc + 1) % n;
            for (int32_t g = 0; g < n && d(pm + 1) < d(pm); ++g) pm = (pm + 1) % n;
        }
        const int64_t d0 = d(pm), d1 = d(pd), c0 = cc(i), c1 = cc(pc), den = ex * ex + ey * ey;
        const i128    num = (i128)(d1 - d0) * (c1 - c0);
        if (best < 0 || num * b_den < b_num * den) {
            best = i; b_ex = ex; b_ey = ey; b_d0 = d0; b_d1 = d1; b_c0 = c0; b_c1 = c1; b_num = num; b_den = den;
        }
    }
    out->hull_area2 = (uint64_t)area2;
    out->edge = best; out->ex = (int32_t)b_ex; out->ey = (int32_t)b_ey;
    out->dmin = b_d0; out->dmax = b_d1; out->cmin = b_c0; out->cmax = b_c1;
    const int64_t dd[4] = {b_d0, b_d1, b_d1, b_d0}, cs[4] = {b_c0, b_c0, b_c1, b_c1};
    for (int k = 0; k < 4; ++k) {
        out->qx[k] = (double)(dd[k] * b_ex - cs[k] * b_ey) / (double)b_den;
        out->qy[k] = (double)(dd[k] * b_ey + cs[k] * b_ex) / (double)b_den;
    }
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

} // extern "C"
