// api_frame_lines.cpp -- the C ABI, part 8: one list of text lines per frame, merged across pyramid levels (STR_ER_WANT_FRAME_LINES in
// run_batch, str_er_line_feet_regions on one host plane) and the result accessors.  What touches no device is in lines_host.cpp
// (str_er_frame_lines_from_pairs, str_er_text_tracks_from_links, the hulls and the oriented boxes) and in words_host.cpp.
// The contract is at str_er_line_foot (str_er.h).  The host lists the members of every line with their pre-image boxes, cuts the
// footprints into jobs and lists the lines of every frame; k_line_foot and k_foot_pairs (er_frame_lines.inl) do the per-pixel work;
// the host sorts the pairs that come back and joins the duplicates (union-find).
// STR_ER_WANT_LINE_LINKS (the contract is at str_er_line_link) rides on the same stage: k_foot_links overlaps the lines of adjacent
// frames behind k_line_foot, beside k_foot_pairs, and shares the stage's upload and wait; the words of the first and of the last
// frame's footprints come back as the result's edge feet; str_er_link_feet runs the same kernel on two uploaded sets of footprints;
// str_er_text_tracks_from_links joins duplicates and links into tracks on the host.
// STR_ER_WANT_LINE_GEOM (the contract is at str_er_line_geom) rides on the same stage as well: k_foot_geom reads every footprint once
// behind k_line_foot and leaves the moments and the hull vertices, which come back in the stage's one wait; the host makes the oriented
// boxes (str_er_quad_from_hull) and merges the hulls of a frame line (str_er_hull_of_points).  str_er_feet_geom runs the same kernel on
// uploaded footprints.
// STR_ER_WANT_LINE_WORDS (the contract is at str_er_line_run) likewise: k_foot_words cuts every footprint into glyph runs behind
// k_line_foot, into (w + 1) / 2 reserved slots a line, which come back in the stage's one wait; the host compacts the slots and forms
// the words (str_er_words_from_runs, words_host.cpp).  str_er_feet_words runs the same kernel on uploaded footprints.
// STR_ER_WANT_RUN_READ behind that, with a second enqueue and wait: run_read_stage (api_run_read.cpp).
#include "str_er_ctx.h"
#include "track_decode_rules.h"
#include "track_read_rules.h"

#include <numeric>

namespace str_er_host {

namespace {

// One member of a line, before the layout: the level size of its plane, its box and where its mask starts
struct FootMember {
    uint32_t line;
    int32_t  pw, ph;
    uint16_t x, y, w, h;
    uint64_t word_off;
};

// The tables of one launch: lines | jobs | list | members | xs / ys tables, and the 64-bit words the footprints take
struct FootTables {
    std::vector<FootLine>    lines;
    std::vector<FootJob>     jobs;
    std::vector<uint32_t>    list;
    std::vector<TextMapCand> members;
    SampleTabs               st;
    uint64_t                 words = 0;
    // with links: per line the lines of the next adjacent frame (into list), and the words [lo, hi) that hold the footprints of the
    // lines of the first ([0]) and of the last frame ([1])
    std::vector<FootRange>   range;
    uint64_t                 edge_lo[2] = {0, 0}, edge_hi[2] = {0, 0};
};

constexpr uint32_t FOOT_JOB_WORDS = 1024;        // 64-bit words of a job of k_line_foot: 16 per lane

// members: ordered by line; frame_of[t]: the frame of line t, frame_wh its level-0 size
void foot_layout(const std::vector<int32_t> &frame_wh, const std::vector<uint32_t> &frame_of, const std::vector<FootMember> &mem, FootTables &T,
                 bool links = false)
{
    const size_t n_lines = frame_of.size(), n_frames = frame_wh.size() / 2;
    T.lines.assign(n_lines, FootLine{});
    std::vector<int32_t> x1(n_lines, 0), y1(n_lines, 0);
    for (const FootMember &g : mem) {
        const int32_t W = frame_wh[2 * frame_of[g.line]], H = frame_wh[2 * frame_of[g.line] + 1];
        TextMapCand C{};
        C.word_off = g.word_off; C.pitch = (g.w + 31u) / 32u; C.x = g.x; C.y = g.y; C.w = g.w; C.h = g.h;
        C.fx0 = first_sample_at(g.x, W, g.pw); C.fx1 = first_sample_at((int64_t)g.x + g.w, W, g.pw);
        C.fy0 = first_sample_at(g.y, H, g.ph); C.fy1 = first_sample_at((int64_t)g.y + g.h, H, g.ph);
        if (C.fx0 >= C.fx1 || C.fy0 >= C.fy1) continue;         // (a plane larger than the frame: no frame pixel samples the box)
        C.xtab = T.st.table(W, g.pw); C.ytab = T.st.table(H, g.ph);
        FootLine &L = T.lines[g.line];
        if (L.count == 0) { L.first = (uint32_t)T.members.size(); L.x = C.fx0; L.y = C.fy0; x1[g.line] = C.fx1; y1[g.line] = C.fy1; }
        L.x = std::min(L.x, C.fx0); L.y = std::min(L.y, C.fy0);
        x1[g.line] = std::max(x1[g.line], C.fx1); y1[g.line] = std::max(y1[g.line], C.fy1);
        ++L.count;
        T.members.push_back(C);
    }
    // the footprints behind one another, cut into jobs of whole rows; the lines of every frame, ascending
    std::vector<uint32_t> per_frame(n_frames + 1, 0);
    for (size_t t = 0; t < n_lines; ++t) {
        FootLine &L = T.lines[t];
        if (L.count == 0) continue;
        L.w = x1[t] - L.x; L.h = y1[t] - L.y;
        L.pitch = ((uint32_t)L.w + 63u) / 64u;
        L.word_off = T.words;
        T.words += (uint64_t)L.h * L.pitch;
        const uint32_t rows = std::max<uint32_t>(1, FOOT_JOB_WORDS / L.pitch);
        for (uint32_t r0 = 0; r0 < (uint32_t)L.h; r0 += rows) T.jobs.push_back(FootJob{(uint32_t)t, r0, std::min(rows, (uint32_t)L.h - r0), 0});
        ++per_frame[frame_of[t] + 1];
    }
    std::partial_sum(per_frame.begin(), per_frame.end(), per_frame.begin());
    T.list.assign(per_frame.back(), 0);
    std::vector<uint32_t> at(per_frame.begin(), per_frame.end() - 1);
    for (size_t t = 0; t < n_lines; ++t) {
        FootLine &L = T.lines[t];
        if (L.count == 0) continue;
        const uint32_t f = frame_of[t];
        T.list[at[f]] = (uint32_t)t;
        L.next = ++at[f]; L.end = per_frame[f + 1];
    }
    if (T.st.tabs.empty()) T.st.tabs.push_back(0);
    if (T.list.empty()) T.list.push_back(0);
    if (!links) return;
    T.range.assign(n_lines, FootRange{0, 0});
    const uint32_t edge[2] = {0, (uint32_t)n_frames - 1};
    bool seen[2] = {false, false};
    for (size_t t = 0; t < n_lines; ++t) {
        const FootLine &L = T.lines[t];
        if (L.count == 0) continue;
        const uint32_t f = frame_of[t];
        if (f + 1 < n_frames && frame_wh[2 * f] == frame_wh[2 * f + 2] && frame_wh[2 * f + 1] == frame_wh[2 * f + 3])
            T.range[t] = FootRange{per_frame[f + 1], per_frame[f + 2]};
        for (int e = 0; e < 2; ++e) {
            if (f != edge[e]) continue;
            const uint64_t lo = L.word_off, hi = L.word_off + (uint64_t)L.h * L.pitch;
            T.edge_lo[e] = seen[e] ? std::min(T.edge_lo[e], lo) : lo;
            T.edge_hi[e] = seen[e] ? std::max(T.edge_hi[e], hi) : hi;
            seen[e] = true;
        }
    }
}

struct FootOut {
    std::vector<FootStat> stat;          // per line
    std::vector<FootPair> pairs;         // inter > 0, sorted by (a, b)
    uint32_t n_candidates = 0;
    size_t   bytes_back = 0;
};

// what the link pass leaves: the overlaps across adjacent frames and the words of the edge frames' footprints (T.edge_lo .. edge_hi)
struct LinkOut {
    std::vector<FootPair> links;         // inter > 0, sorted by (a, b)
    std::vector<uint64_t> edge[2];
    uint32_t n_candidates = 0;
    size_t   bytes_back = 0, edge_bytes = 0;
};

void sort_pairs(std::vector<FootPair> &v)
{
    std::sort(v.begin(), v.end(), [](const FootPair &p, const FootPair &q) { return p.a != q.a ? p.a < q.a : p.b < q.b; });
}

// A counted table of FootPair behind a FootHead in a device / page-locked pair: the head at 0, the records from o_rec on (between them
// the pairs' per-line statistics), and behind the records of the first pass `tail` more bytes of the page-locked side (the links' edge
// words).  A pass: enqueue, the caller's wait, collect -- which asks for one more pass when the table was too small.
struct PairTable {
    PairBuf    &buf;
    const char *what, *twice;         // the buffer's name, and the error of a second overflow
    size_t      o_rec = sizeof(FootHead);
    size_t      cap = 0;
    bool        grown = false;
    uint32_t    n_candidates = 0;
    size_t      bytes_back = 0;

    size_t back() const { return o_rec + sizeof(FootPair) * cap; }         // what a pass copies back: the head and cap records
    // the first capacity for a launch over n_lines lines: max(1024, 4 n_lines) records, and as many as the buffer already holds
    int reserve(str_er_ctx *c, size_t n_lines, size_t tail = 0)
    {
        cap = std::max<size_t>(1024, 4 * n_lines);
        if (buf.size() > o_rec + tail) cap = std::max(cap, (buf.size() - o_rec - tail) / sizeof(FootPair));
        return buf.ensure(c, back() + tail, what);
    }
    // launch(head, records, cap): the kernel that counts into the zeroed head and fills the records
    template <typename Launch> int enqueue(str_er_ctx *c, hipStream_t s, Launch launch)
    {
        HIP_TRY(c, hipMemsetAsync(buf.d(), 0, sizeof(FootHead), s));
        launch(buf.d<FootHead>(), reinterpret_cast<FootPair *>(buf.d() + o_rec), (uint32_t)cap);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(buf.h(), buf.d(), back(), hipMemcpyDeviceToHost, s));
        bytes_back += back();
        return STR_ER_OK;
    }
    // after the wait: the records into out; again: there were more than the table holds -- it now holds them all (whatever else was in
    // the buffer is lost), and the pass is to run once more (what it reads is still on the device)
    int collect(str_er_ctx *c, std::vector<FootPair> &out, bool &again)
    {
        FootHead head;
        std::memcpy(&head, buf.h(), sizeof head);
        n_candidates = head.n_candidates;
        again = head.n_pairs > cap;
        if (!again) {
            out.resize(head.n_pairs);
            if (head.n_pairs) std::memcpy(out.data(), buf.h() + o_rec, sizeof(FootPair) * head.n_pairs);
            return STR_ER_OK;
        }
        if (grown) return fail(c, STR_ER_EHIP, twice);
        grown = true;
        cap = head.n_pairs;
        return buf.ensure(c, back(), what);
    }
};

PairTable link_table(str_er_ctx *c) { return {c->link_out, "line link output", "line links: the link table overflowed twice (internal error)"}; }


// n rows for a caller's array of cap rows; what: "pairs, cap_pairs"
int check_cap(str_er_ctx *c, size_t n, int64_t cap, const char *what)
{
    return (int64_t)n > cap ? fail(c, STR_ER_ECAPACITY, std::to_string(n) + " " + what + " is " + std::to_string(cap)) : STR_ER_OK;
}

// ... and copied into it; dst == null: the caller asked for the count alone
int copy_out(str_er_ctx *c, const void *src, size_t n, size_t row_bytes, void *dst, int64_t cap, const char *what)
{
    if (!dst) return STR_ER_OK;
    if (const int rc = check_cap(c, n, cap, what); rc != STR_ER_OK) return rc;
    if (n) std::memcpy(dst, src, row_bytes * n);
    return STR_ER_OK;
}

constexpr int32_t GEOM_MAX_BOX = 16384;          // the widest / tallest foot box whose moments are promised not to overflow

// The feet and footprints a caller hands in (str_er_link_feet: two sets behind one another; str_er_feet_geom, str_er_feet_words,
// str_er_feet_read: one): checked, packed into a table of lines and rows of 64-bit words, and uploaded into c->foot_tab (the lines
// first) and c->foot_bits on c->stream.  It owns the host words, which the queued upload reads: whoever leaves the scope before a wait
// of the stream has succeeded (wait) -- an enqueue that failed behind the upload -- drains the stream first.
struct CallerFeet {
    str_er_ctx           *c;
    std::vector<FootLine> lines;
    std::vector<uint64_t> words;
    bool                  queued = false;

    explicit CallerFeet(str_er_ctx *ctx) : c(ctx) {}
    ~CallerFeet() { if (queued) (void)hipStreamSynchronize(c->stream); }

    // the boxes of all feet of a set; who: in front of "line t"
    int check_boxes(int32_t W, int32_t H, const str_er_line_foot *feet, int32_t n, const char *who)
    {
        for (int32_t t = 0; t < n; ++t) {
            const str_er_line_foot &F = feet[t];
            const std::string line = who + ("line " + std::to_string(t));
            if (F.w < 0 || F.h < 0 || (F.w == 0) != (F.h == 0)) return fail(c, STR_ER_EINVAL, line + ": bad foot box");
            if (F.w == 0) {
                if (F.pixels) return fail(c, STR_ER_EINVAL, line + ": pixels in an empty foot box");
                continue;
            }
            if (F.x < 0 || F.y < 0 || (int64_t)F.x + F.w > W || (int64_t)F.y + F.h > H) return fail(c, STR_ER_EINVAL, line + ": the foot box leaves the frame");
        }
        return STR_ER_OK;
    }
    // ... against the largest box the kernel behind takes (GEOM_MAX_BOX, WORDS_MAX_BOX)
    int check_limit(const str_er_line_foot *feet, int32_t n, int32_t max_box)
    {
        for (int32_t t = 0; t < n; ++t)
            if (feet[t].w > max_box || feet[t].h > max_box)
                return fail(c, STR_ER_ECAPACITY, "line " + std::to_string(t) + ": a foot box wider or taller than " + std::to_string(max_box) + " pixels");
        return STR_ER_OK;
    }
    // ... then the footprints of the set (rows of 32-bit words behind one another in bits) appended to lines / words as rows of 64-bit
    // words, every one checked against its foot.  blank_empty: a box without a bit is an empty footprint (a zeroed line)
    int pack(const str_er_line_foot *feet, const uint32_t *bits, int32_t n, bool blank_empty)
    {
        const uint32_t *at = bits;
        for (int32_t t = 0; t < n; ++t) {
            const str_er_line_foot &F = feet[t];
            FootLine L{};
            L.word_off = words.size();
            if (F.w != 0) {
                if (!at) return fail(c, STR_ER_EINVAL, "footprint bits missing");
                L.x = F.x; L.y = F.y; L.w = F.w; L.h = F.h; L.pitch = ((uint32_t)F.w + 63u) / 64u; L.count = 1;
                const uint32_t pitch32 = ((uint32_t)F.w + 31u) / 32u, tail = (uint32_t)F.w & 31u;
                uint64_t px = 0;
                for (int32_t rr = 0; rr < F.h; ++rr, at += pitch32) {
                    if (tail && (at[pitch32 - 1] >> tail)) return fail(c, STR_ER_EINVAL, "a footprint has a bit set past its row's width");
                    for (uint32_t k = 0; k < L.pitch; ++k) {
                        const uint64_t v = (uint64_t)at[2 * k] | (2 * k + 1 < pitch32 ? (uint64_t)at[2 * k + 1] << 32 : 0ull);
                        px += (uint64_t)__builtin_popcountll(v);
                        words.push_back(v);
                    }
                }
                if (px != F.pixels) return fail(c, STR_ER_EINVAL, "a foot's pixels are not the number of bits set in its footprint");
            }
            lines.push_back(blank_empty && F.pixels == 0 ? FootLine{} : L);
        }
        return STR_ER_OK;
    }
    // room for tab_need bytes of tables and for the words; the caller puts what lies behind the lines into c->foot_tab.h() ...
    int reserve(size_t tab_need)
    {
        HIP_TRY(c, hipSetDevice(c->prm.device));
        const int rc = c->foot_tab.ensure(c, tab_need, "frame line tables");
        return rc != STR_ER_OK ? rc : c->foot_bits.ensure(c, 8 * words.size(), "line footprints");
    }
    // ... and both are on their way
    int upload(size_t tab_need)
    {
        hipStream_t s = c->stream;
        std::memcpy(c->foot_tab.h(), lines.data(), sizeof(FootLine) * lines.size());
        HIP_TRY(c, hipMemcpyAsync(c->foot_tab.d(), c->foot_tab.h(), tab_need, hipMemcpyHostToDevice, s));
        queued = true;
        HIP_TRY(c, hipMemcpyAsync(c->foot_bits.d<uint64_t>(), words.data(), 8 * words.size(), hipMemcpyHostToDevice, s));
        return STR_ER_OK;
    }
    int wait()
    {
        hipStream_t s = c->stream;
        HIP_TRY(c, wait_stream(c, s));
        queued = false;
        return STR_ER_OK;
    }
    const FootLine *d_lines() const { return reinterpret_cast<const FootLine *>(c->foot_tab.d()); }
};

// One per-line side pass behind the footprints in c->foot_bits (k_foot_geom, k_foot_words): a slot per line that tells the kernel
// where the line's elements go, a record per line that the kernel leaves, and the elements (hull vertices, run slots), in one buffer
// laid out as slots | records | elements (the same on both sides).  enqueue; the caller's wait; then the records and elements are
// on the page-locked side.
template <typename Slot, typename Rec, size_t ELEM> struct LinePass {
    PairBuf    &buf;
    const char *what, *too_many;          // the buffer's name, and the error of more than 2^31 elements
    DevBuf     *extra = nullptr;          // a second buffer of the kernel's, of extra_bytes (the slot rule counts them)
    const char *extra_what = nullptr;
    size_t      extra_bytes = 0;
    std::vector<Slot> slots;
    size_t      n_lines = 0, n_elems = 0, o_rec = 0, o_elem = 0, bytes = 0;

    bool   launched() const { return bytes != 0; }
    size_t bytes_back() const { return bytes - o_rec; }
    Rec    rec(size_t t) const { Rec R; std::memcpy(&R, buf.h() + o_rec + sizeof(Rec) * t, sizeof R); return R; }
    const uint8_t *elems() const { return buf.h() + o_elem; }

    // rule(L, slot, first): fills the slot of a line with a footprint, whose elements start at `first`, and returns how many it reserves;
    // launch(slots, records, elements): the kernel, on the device side.  The slots uploaded, the kernel and the copy back enqueued on s.
    template <typename Rule, typename Launch> int enqueue(str_er_ctx *c, hipStream_t s, const std::vector<FootLine> &lines, Rule rule, Launch launch)
    {
        n_lines = lines.size();
        slots.assign(n_lines, Slot{0, 0});
        uint64_t at = 0;
        for (size_t t = 0; t < n_lines; ++t) {
            const FootLine &L = lines[t];
            if (L.w <= 0 || L.h <= 0) continue;
            at += rule(L, slots[t], (uint32_t)at);
            if (at > 0x7FFFFFFFull) return fail(c, STR_ER_ECAPACITY, too_many);
        }
        n_elems = (size_t)at;
        if (n_lines == 0) return STR_ER_OK;
        o_rec = align_up(sizeof(Slot) * n_lines, 256); o_elem = align_up(o_rec + sizeof(Rec) * n_lines, 256);
        bytes = o_elem + ELEM * n_elems;
        int rc = buf.ensure(c, bytes, what);
        if (rc != STR_ER_OK || (extra && (rc = extra->ensure(c, extra_bytes, extra_what)) != STR_ER_OK)) return rc;
        std::memcpy(buf.h(), slots.data(), sizeof(Slot) * n_lines);
        HIP_TRY(c, hipMemcpyAsync(buf.d(), buf.h(), sizeof(Slot) * n_lines, hipMemcpyHostToDevice, s));
        launch(reinterpret_cast<const Slot *>(buf.d()), reinterpret_cast<Rec *>(buf.d() + o_rec), buf.d() + o_elem);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(buf.h() + o_rec, buf.d() + o_rec, bytes - o_rec, hipMemcpyDeviceToHost, s));
        return STR_ER_OK;
    }
};

static_assert(sizeof(WordsRun) == sizeof(str_er_line_run), "the device writes str_er_line_run records");
using GeomPass = LinePass<GeomSlot, GeomRec, 8>;                          // elements: hull vertices, x and y
using WordsPass = LinePass<WordsSlot, WordsRec, sizeof(WordsRun)>;        // elements: run slots

GeomPass geom_pass(str_er_ctx *c)
{
    return {c->geom_out, "line geometry output", "line geometry: more than 2^31 hull vertices to reserve", &c->geom_x, "line geometry rows"};
}
WordsPass words_pass(str_er_ctx *c) { return {c->words_out, "line words output", "line words: more than 2^31 glyph runs to reserve"}; }

// k_foot_geom over the lines of a launch, behind whatever made their footprints; geom_collect after the wait
int geom_enqueue(str_er_ctx *c, hipStream_t s, const std::vector<FootLine> &lines, const FootLine *d_lines, GeomPass &P)
{
    return P.enqueue(
        c, s, lines,
        [&](const FootLine &L, GeomSlot &S, uint32_t first) {
            S.pt_first = first;
            if (L.h + 1 > GEOM_LDS_ROWS) { S.x_first = (uint32_t)(P.extra_bytes / 8); P.extra_bytes += 8 * ((size_t)L.h + 1u); }         // (its scratch rows)
            return 2ull * ((uint64_t)L.h + 1u);          // (a chain has at most one vertex per height 0 .. h)
        },
        [&](const GeomSlot *slots, GeomRec *recs, uint8_t *xy) {
            launch_foot_geom(s, d_lines, (int)lines.size(), slots, c->foot_bits.d<uint64_t>(), c->geom_x.d<uint64_t>(), recs, reinterpret_cast<int32_t *>(xy));
        });
}

// after the wait: one record per line (n_lines of them), its vertices appended to xy (x, y pairs) and its box made
// (str_er_quad_from_hull).  Nothing was launched (no footprint at all): every line is empty
int geom_collect(str_er_ctx *c, const GeomPass &P, size_t n_lines, std::vector<str_er_line_geom> &geoms, std::vector<int32_t> &xy)
{
    geoms.assign(n_lines, str_er_line_geom{});
    for (str_er_line_geom &G : geoms) G.edge = -1;
    if (!P.launched()) return STR_ER_OK;
    for (size_t t = 0; t < n_lines; ++t) {
        str_er_line_geom &G = geoms[t];
        const GeomRec R = P.rec(t);
        if (R.count == 0) continue;
        const uint32_t first = P.slots[t].pt_first;
        if (R.count < 4 || (size_t)first + R.count > P.n_elems) return fail(c, STR_ER_EHIP, "line geometry: a hull outside its vertices (internal error)");
        const int32_t *src = reinterpret_cast<const int32_t *>(P.elems()) + 2 * (size_t)first;
        G.first = (uint32_t)(xy.size() / 2); G.count = R.count;
        xy.insert(xy.end(), src, src + 2 * (size_t)R.count);
        G.pixels = R.pixels; G.m10 = R.m10; G.m01 = R.m01; G.m20 = R.m20; G.m11 = R.m11; G.m02 = R.m02;
        if (str_er_quad_from_hull(xy.data() + 2 * (size_t)G.first, (int32_t)G.count, &G) != STR_ER_OK)
            return fail(c, STR_ER_EHIP, "line geometry: the device's hull is not a hull (internal error)");
    }
    return STR_ER_OK;
}

// a footprint box k_foot_words does not take (checked before anything is enqueued); who: in front of the message
int words_check_boxes(str_er_ctx *c, const std::vector<FootLine> &lines, const char *who)
{
    for (const FootLine &L : lines)
        if (L.w > WORDS_MAX_BOX || L.h > WORDS_MAX_BOX)
            return fail(c, STR_ER_ECAPACITY, std::string(who) + "a footprint wider or taller than " + std::to_string(WORDS_MAX_BOX) + " pixels");
    return STR_ER_OK;
}

// k_foot_words over the lines of a launch, behind whatever made their footprints; words_collect after the wait
int words_enqueue(str_er_ctx *c, hipStream_t s, const std::vector<FootLine> &lines, const FootLine *d_lines, WordsPass &P)
{
    return P.enqueue(
        c, s, lines,
        [](const FootLine &L, WordsSlot &S, uint32_t first) {
            S = WordsSlot{first, ((uint32_t)L.w + 1u) / 2u};          // (the most runs a row of w columns holds)
            return (uint64_t)S.cap;
        },
        [&](const WordsSlot *slots, WordsRec *recs, uint8_t *runs) {
            launch_foot_words(s, d_lines, (int)lines.size(), slots, c->foot_bits.d<uint64_t>(), recs, reinterpret_cast<WordsRun *>(runs));
        });
}

// after the wait: the slots compacted into runs (back to back in line order), one record per line (n_lines of them), and the words
// formed (str_er_words_from_runs with the context's gap).  Nothing was launched (no footprint at all): no runs and no words
int words_collect(str_er_ctx *c, const WordsPass &P, size_t n_lines, std::vector<str_er_line_words> &line_words, std::vector<str_er_line_run> &runs,
                  std::vector<str_er_line_word> &words)
{
    line_words.assign(n_lines, str_er_line_words{});
    runs.clear(); words.clear();
    if (!P.launched()) return STR_ER_OK;
    for (size_t t = 0; t < n_lines; ++t) {
        const WordsRec R = P.rec(t);
        if (R.n_runs > P.slots[t].cap || (R.n_runs == 0) != (R.colmax == 0))
            return fail(c, STR_ER_EHIP, "line words: a line's runs outside its slots (internal error)");
        str_er_line_words &LW = line_words[t];
        LW.first_run = (int32_t)runs.size(); LW.n_runs = (int32_t)R.n_runs; LW.colmax = R.colmax;
        if (R.n_runs == 0) continue;
        runs.resize(runs.size() + R.n_runs);
        std::memcpy(runs.data() + LW.first_run, P.elems() + sizeof(WordsRun) * P.slots[t].first, sizeof(WordsRun) * R.n_runs);
    }
    if (runs.size() > 0x7FFFFFFFull) return fail(c, STR_ER_ECAPACITY, "line words: more than 2^31 glyph runs");
    words.resize(runs.size());
    int32_t n_words = 0;
    if (str_er_words_from_runs(runs.data(), (int32_t)runs.size(), line_words.data(), (int32_t)n_lines, c->word_num, c->word_den, words.data(),
                               (int32_t)words.size(), &n_words) != STR_ER_OK)
        return fail(c, STR_ER_EHIP, "line words: the device's runs are not runs (internal error)");
    words.resize((size_t)n_words);
    return STR_ER_OK;
}

// what a stage leaves behind its wait: the pairs, and what rode along (LineStageWants)
struct StageOut {
    FootOut   feet;
    LinkOut   links;
    GeomPass  geom;
    WordsPass words;
    explicit StageOut(str_er_ctx *c) : geom(geom_pass(c)), words(words_pass(c)) {}
};

// one upload, the launches on s, one copy back, one wait (a pair pass again, with a larger table, if its pairs outgrew it).
// want.links: the links across adjacent frames as well (T.range), in the same upload and wait, with a table and a copy of their own
// want.geom: the geometry of the footprints as well (k_foot_geom behind k_line_foot, its copy back ahead of the same wait; geom_collect afterwards)
// want.words: their glyph runs as well (k_foot_words, in the same way; words_collect afterwards)
int foot_stage(str_er_ctx *c, hipStream_t s, const FootTables &T, const uint32_t *d_bits, bool in_batch, const LineStageWants &want, StageOut &S)
{
    FootOut &O = S.feet;
    LinkOut *LK = want.links ? &S.links : nullptr;
    const size_t n_lines = T.lines.size();
    O.stat.assign(n_lines, FootStat{});
    O.pairs.clear();
    if (T.members.empty()) return STR_ER_OK;
    const size_t o_jobs = align_up(sizeof(FootLine) * n_lines, 256), o_list = align_up(o_jobs + sizeof(FootJob) * T.jobs.size(), 256);
    const size_t o_mem = align_up(o_list + 4 * T.list.size(), 256), o_tab = align_up(o_mem + sizeof(TextMapCand) * T.members.size(), 256);
    const size_t o_rng = LK ? align_up(o_tab + 2 * T.st.tabs.size(), 256) : 0;
    const size_t tab_need = LK ? o_rng + sizeof(FootRange) * n_lines : o_tab + 2 * T.st.tabs.size();
    int rc = c->foot_tab.ensure(c, tab_need, "frame line tables");
    if (rc != STR_ER_OK || (rc = c->foot_bits.ensure(c, 8 * (size_t)T.words, "line footprints")) != STR_ER_OK) return rc;
    const size_t o_stat = sizeof(FootHead);
    PairTable PT{c->foot_out, "frame line output", "frame lines: the pair table overflowed twice (internal error)", o_stat + sizeof(FootStat) * n_lines};
    PairTable LT = link_table(c);
    if ((rc = PT.reserve(c, n_lines)) != STR_ER_OK) return rc;
    std::memcpy(c->foot_tab.h(), T.lines.data(), sizeof(FootLine) * n_lines);
    if (!T.jobs.empty()) std::memcpy(c->foot_tab.h() + o_jobs, T.jobs.data(), sizeof(FootJob) * T.jobs.size());
    std::memcpy(c->foot_tab.h() + o_list, T.list.data(), 4 * T.list.size());
    std::memcpy(c->foot_tab.h() + o_mem, T.members.data(), sizeof(TextMapCand) * T.members.size());
    std::memcpy(c->foot_tab.h() + o_tab, T.st.tabs.data(), 2 * T.st.tabs.size());
    // the links: the edge frames' words (one range when the call is one frame) lie behind the link table on the page-locked side
    const bool   one_edge = LK && T.edge_lo[0] == T.edge_lo[1] && T.edge_hi[0] == T.edge_hi[1];
    const size_t edge_n[2] = {LK ? (size_t)(T.edge_hi[0] - T.edge_lo[0]) : 0, LK && !one_edge ? (size_t)(T.edge_hi[1] - T.edge_lo[1]) : 0};
    if (LK) {
        LK->edge_bytes = 8 * (edge_n[0] + edge_n[1]);
        if ((rc = LT.reserve(c, n_lines, LK->edge_bytes)) != STR_ER_OK) return rc;
        std::memcpy(c->foot_tab.h() + o_rng, T.range.data(), sizeof(FootRange) * n_lines);
    }
    HIP_TRY(c, hipMemcpyAsync(c->foot_tab.d(), c->foot_tab.h(), tab_need, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(c->foot_out.d() + o_stat, 0, sizeof(FootStat) * n_lines, s));
    const FootLine *d_lines = reinterpret_cast<const FootLine *>(c->foot_tab.d());
    const uint32_t *d_list = reinterpret_cast<const uint32_t *>(c->foot_tab.d() + o_list);
    uint64_t       *feet = c->foot_bits.d<uint64_t>();
    launch_line_foot(s, reinterpret_cast<const FootJob *>(c->foot_tab.d() + o_jobs), (int)T.jobs.size(), d_lines,
                     reinterpret_cast<const TextMapCand *>(c->foot_tab.d() + o_mem), reinterpret_cast<const uint16_t *>(c->foot_tab.d() + o_tab), d_bits,
                     feet, reinterpret_cast<FootStat *>(c->foot_out.d() + o_stat));
    HIP_TRY(c, hipGetLastError());
    if (LK) {
        uint8_t *h_edge = c->link_out.h() + LT.back();
        for (int e = 0; e < 2; ++e) {
            if (edge_n[e]) HIP_TRY(c, hipMemcpyAsync(h_edge, feet + T.edge_lo[e], 8 * edge_n[e], hipMemcpyDeviceToHost, s));
            h_edge += 8 * edge_n[e];
        }
    }
    if (want.geom && (rc = geom_enqueue(c, s, T.lines, d_lines, S.geom)) != STR_ER_OK) return rc;
    if (want.words && (rc = words_enqueue(c, s, T.lines, d_lines, S.words)) != STR_ER_OK) return rc;
    // (k_run_cuts directly behind k_foot_words, on its run slots: its records come down with this stage's wait)
    if (want.words && want.split &&
        (rc = run_cuts_enqueue(c, s, d_lines, (int32_t)n_lines, S.words.buf.d(), S.words.o_rec, S.words.o_elem, S.words.n_elems)) != STR_ER_OK)
        return rc;
    const auto launch_pairs = [&](FootHead *head, FootPair *out, uint32_t cap) { launch_foot_pairs(s, d_lines, (int)n_lines, d_list, feet, head, out, cap); };
    const auto launch_links = [&](FootHead *head, FootPair *out, uint32_t cap) {
        launch_foot_links(s, d_lines, (int)n_lines, reinterpret_cast<const FootRange *>(c->foot_tab.d() + o_rng), d_list, feet, head, out, cap);
    };
    bool run_pairs = true, run_links = LK != nullptr;
    for (bool first = true; run_pairs || run_links; first = false) {
        // what comes back: the counters, the statistics and the pairs in one copy (the table is sized for four pairs a line: all of it is a
        // few hundred KB at most for a batch; the host reads as many as the counter says); the links' counters and table in another
        if (run_pairs && (rc = PT.enqueue(c, s, launch_pairs)) != STR_ER_OK) return rc;
        if (run_links && (rc = LT.enqueue(c, s, launch_links)) != STR_ER_OK) return rc;
        if (in_batch && first) rec(c, "frame_lines");          // (the call's one profiling event of the stage)
        HIP_TRY(c, wait_stream(c, s));
        if (first) std::memcpy(O.stat.data(), c->foot_out.h() + o_stat, sizeof(FootStat) * n_lines);
        if (first && LK) {         // (before the link table may grow: the edge words lie in the same buffer)
            const uint8_t *h_edge = c->link_out.h() + LT.back();
            LK->edge[0].resize(edge_n[0]);
            if (edge_n[0]) std::memcpy(LK->edge[0].data(), h_edge, 8 * edge_n[0]);
            LK->edge[1].resize(edge_n[1]);
            if (edge_n[1]) std::memcpy(LK->edge[1].data(), h_edge + 8 * edge_n[0], 8 * edge_n[1]);
            if (one_edge) LK->edge[1] = LK->edge[0];
        }
        if (run_pairs && (rc = PT.collect(c, O.pairs, run_pairs)) != STR_ER_OK) return rc;
        if (run_links && (rc = LT.collect(c, LK->links, run_links)) != STR_ER_OK) return rc;
    }
    O.n_candidates = PT.n_candidates; O.bytes_back = PT.bytes_back;
    if (LK) { LK->n_candidates = LT.n_candidates; LK->bytes_back = LT.bytes_back; }
    sort_pairs(O.pairs);
    if (LK) sort_pairs(LK->links);
    return STR_ER_OK;
}

void feet_from_stats(const std::vector<FootStat> &stat, std::vector<str_er_line_foot> &feet)
{
    feet.assign(stat.size(), str_er_line_foot{});
    for (size_t t = 0; t < stat.size(); ++t) {
        const FootStat &S = stat[t];
        str_er_line_foot &F = feet[t];
        F.frame_line = -1;
        if (S.pixels == 0) continue;
        F.x = (int32_t)(65536u - S.nx0); F.y = (int32_t)(65536u - S.ny0);
        F.w = (int32_t)S.x1 - F.x; F.h = (int32_t)S.y1 - F.y;
        F.pixels = S.pixels;
    }
}

static_assert(sizeof(FootPair) == sizeof(str_er_line_pair), "the device writes str_er_line_pair records");
static_assert(sizeof(FootPair) == sizeof(str_er_line_link), "the device writes str_er_line_link records");

// a footprint as it lies on the device (rows of L.pitch 64-bit words over L's box, the first at `words`), cut to the foot box F and
// appended to out as rows of (F.w + 31) / 32 32-bit words
void foot_rows32(const uint64_t *words, const FootLine &L, const str_er_line_foot &F, std::vector<uint32_t> &out)
{
    const uint32_t pitch32 = ((uint32_t)F.w + 31u) / 32u;
    for (int32_t rr = 0; rr < F.h; ++rr) {
        const uint64_t *row = words + (uint64_t)(F.y - L.y + rr) * L.pitch;
        for (uint32_t k = 0; k < pitch32; ++k) {
            const uint32_t off = (uint32_t)(F.x - L.x) + 32u * k, q = off >> 6, sh = off & 63u;
            uint64_t v = q < L.pitch ? row[q] >> sh : 0ull;
            if (sh && q + 1 < L.pitch) v |= row[q + 1] << (64u - sh);
            out.push_back((uint32_t)v);
        }
    }
}

// The steps of frame_lines_phase.  The members of every line of r, each once, and where their masks start on the device (d_bits): this
// call's mask words (d_mask_bits / word_off), or made here by the mask kernels and left on the device
int gather_members(str_er_ctx *c, hipStream_t s, const Batch &b, float qscale, const uint32_t *d_mask_bits, const std::vector<uint64_t> *word_off,
                   const str_er_result *r, std::vector<uint32_t> &frame_of, std::vector<uint8_t> &pyr_of, std::vector<FootMember> &mem, const uint32_t *&d_bits)
{
    const size_t n_frames = b.frame_wh.size() / 2, n_lines = r->texts.size();
    frame_of.resize(n_lines); pyr_of.resize(n_lines);
    std::vector<uint32_t> who;             // candidate of every member
    std::vector<int32_t>  ers;
    for (size_t t = 0; t < n_lines; ++t) {
        const str_er_text &tx = r->texts[t];
        if (tx.frame >= n_frames) return fail(c, STR_ER_EHIP, "frame lines: a line of no frame (internal error)");
        frame_of[t] = tx.frame; pyr_of[t] = tx.pyr;
        ers.assign(r->text_ers.begin() + tx.first, r->text_ers.begin() + tx.first + tx.count);
        std::sort(ers.begin(), ers.end());
        ers.erase(std::unique(ers.begin(), ers.end()), ers.end());
        for (const int32_t k : ers) {
            const str_er_cand &cd = r->cands[(size_t)k];
            const PlaneDesc   &pd = b.planes[cd.plane];
            if (cd.w > MASK_MAX_WIDTH) return fail(c, STR_ER_ECAPACITY, "STR_ER_WANT_FRAME_LINES: a candidate wider than " + std::to_string(MASK_MAX_WIDTH) + " pixels");
            FootMember g{};
            g.line = (uint32_t)t; g.pw = pd.w; g.ph = pd.h; g.x = cd.x; g.y = cd.y; g.w = cd.w; g.h = cd.h;
            mem.push_back(g);
            who.push_back((uint32_t)k);
        }
    }
    d_bits = d_mask_bits;
    if (d_mask_bits && word_off) {
        for (size_t i = 0; i < mem.size(); ++i) {
            mem[i].word_off = (*word_off)[who[i]];
            if (mem[i].word_off == UINT64_MAX) return fail(c, STR_ER_EHIP, "frame lines: a member without a mask (internal error)");
        }
    } else if (!mem.empty()) {
        std::vector<uint32_t> uniq(who);
        std::sort(uniq.begin(), uniq.end());
        uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
        std::vector<MaskJob>  mj(uniq.size());
        std::vector<uint64_t> off_of(uniq.size());
        uint64_t words = 0;
        for (size_t i = 0; i < uniq.size(); ++i) {
            const str_er_cand &cd = r->cands[uniq[i]];
            const PlaneDesc   &pd = b.planes[cd.plane];
            MaskJob &m = mj[i];
            m.pix = pd.pix; m.stride = pd.stride; m.invert = (uint32_t)pd.invert; m.plane_w = (uint32_t)pd.w; m.key = cd.key;
            m.x = cd.x; m.y = cd.y; m.w = cd.w; m.h = cd.h; m.level = cd.level; m.idx = (uint32_t)i; m.out_off = words; m.scratch_off = 0;
            off_of[i] = words;
            words += (uint64_t)cd.h * ((cd.w + 31u) / 32u);
        }
        const int rcm = mask_launch(c, s, mj, words, qscale, &d_bits);
        if (rcm != STR_ER_OK) return rcm;
        for (size_t i = 0; i < mem.size(); ++i)
            mem[i].word_off = off_of[(size_t)(std::lower_bound(uniq.begin(), uniq.end(), who[i]) - uniq.begin())];
    }
    return STR_ER_OK;
}

// the pairs, the frame lines and their members from the feet and the stage's pairs; n_fl: the number of frame lines
int fill_frame_lines(str_er_ctx *c, str_er_result *r, const std::vector<uint32_t> &frame_of, const std::vector<uint8_t> &pyr_of, const std::vector<FootPair> &pairs,
                     int32_t &n_fl)
{
    const size_t n_lines = frame_of.size();
    r->line_pairs.resize(pairs.size());
    if (!pairs.empty()) std::memcpy(r->line_pairs.data(), pairs.data(), sizeof(FootPair) * pairs.size());
    r->frame_lines.resize(n_lines);
    r->frame_line_members.resize(n_lines);
    const int rcf = str_er_frame_lines_from_pairs(r->line_feet.data(), frame_of.data(), pyr_of.data(), (int32_t)n_lines, r->line_pairs.data(),
                                                  (int32_t)r->line_pairs.size(), c->merge_num, c->merge_den, r->frame_lines.data(), (int32_t)n_lines, &n_fl,
                                                  r->frame_line_members.data());
    if (rcf != STR_ER_OK) return fail(c, STR_ER_EHIP, "frame lines: the device's pairs do not fit its footprints (internal error)");
    r->frame_lines.resize((size_t)n_fl);
    r->have_frame_lines = true;
    return STR_ER_OK;
}

// the links, the tracks and the edge feet: the lines of the first and of the last frame, their feet and their footprints cut to the foot boxes
int fill_links(str_er_ctx *c, const Batch &b, str_er_result *r, const std::vector<uint32_t> &frame_of, const FootTables &T, const LinkOut &LK)
{
    const size_t n_frames = b.frame_wh.size() / 2, n_lines = frame_of.size();
    r->line_links.resize(LK.links.size());
    if (!LK.links.empty()) std::memcpy(r->line_links.data(), LK.links.data(), sizeof(FootPair) * LK.links.size());
    r->line_tracks.resize(n_lines);
    r->text_tracks.resize(n_lines);
    r->text_track_members.resize(n_lines);
    int32_t n_tr = 0;
    const int rct = str_er_text_tracks_from_links(r->line_feet.data(), frame_of.data(), (int32_t)n_lines, r->line_pairs.data(), (int32_t)r->line_pairs.size(),
                                                  r->line_links.data(), (int32_t)r->line_links.size(), c->link_num, c->link_den, r->line_tracks.data(),
                                                  r->text_tracks.data(), (int32_t)n_lines, &n_tr, r->text_track_members.data());
    if (rct != STR_ER_OK) return fail(c, STR_ER_EHIP, "line links: the device's links do not fit its footprints (internal error)");
    r->text_tracks.resize((size_t)n_tr);
    for (int e = 0; e < 2; ++e) {
        str_er_result::EdgeFeet &E = r->edge_feet[e];
        const uint32_t f = e == 0 ? 0u : (uint32_t)n_frames - 1u;
        E = str_er_result::EdgeFeet{};
        if (n_frames == 0) continue;
        E.w = b.frame_wh[2 * f]; E.h = b.frame_wh[2 * f + 1];
        for (size_t t = 0; t < n_lines; ++t) {
            if (frame_of[t] != f) continue;
            E.lines.push_back((int32_t)t);
            E.feet.push_back(r->line_feet[t]);
            if (r->line_feet[t].pixels) foot_rows32(LK.edge[e].data() + (T.lines[t].word_off - T.edge_lo[e]), T.lines[t], r->line_feet[t], E.bits);
        }
    }
    r->have_line_links = true;
    if (c->dbg_stats)        // developer aid (tools/dev_line_links.py)
        std::fprintf(stderr, "[str_er] line links: %u candidate pairs, %zu overlaps, %d tracks, %zu bytes back for the link table, %zu bytes back for the edge feet\n",
                     LK.n_candidates, LK.links.size(), n_tr, LK.bytes_back, LK.edge_bytes);
    return STR_ER_OK;
}

// the geometry of the lines (what k_foot_geom left) and of the frame lines (frame_line_geoms, lines_host.cpp)
int fill_geometry(str_er_ctx *c, str_er_result *r, const GeomPass &GP)
{
    const auto   t2 = std::chrono::steady_clock::now();
    const size_t n_lines = r->line_feet.size();
    r->geom_points.clear();
    if (const int rcg = geom_collect(c, GP, n_lines, r->line_geoms, r->geom_points); rcg != STR_ER_OK) return rcg;
    if (frame_line_geoms(r->frame_lines.data(), r->frame_lines.size(), r->frame_line_members.data(), r->line_geoms.data(), r->geom_points, r->frame_line_geoms) !=
        STR_ER_OK)
        return fail(c, STR_ER_EHIP, "line geometry: the hull of a frame line failed (internal error)");
    r->have_line_geom = true;
    if (c->dbg_stats)        // developer aid (tools/dev_line_geom.py)
        std::fprintf(stderr, "[str_er] line geometry: %zu lines, %zu vertices reserved, %zu kept, %zu bytes back, host %.3f ms\n", n_lines, GP.n_elems,
                     r->geom_points.size() / 2, GP.bytes_back(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count());
    return STR_ER_OK;
}

// the runs and words of the lines (what k_foot_words left), and with read the reading of every run: T.lines is the table k_foot_words
// read, and its footprints are still in c->foot_bits
// track: the word links and word tracks of STR_ER_WANT_TRACK_READ on the host before the reading (the text tracks of r are made: fill_links),
// the track match behind the matcher, with ltrack the one over the members' piece lattices behind the lattice match (frame_of: the frame of every line, frame_wh: the level-0 sizes of the frames)
// tdecode: the same links and tracks for STR_ER_WANT_TRACK_DECODE (made once where both flags are set), the track decode behind the decoder
int fill_words(str_er_ctx *c, hipStream_t s, str_er_result *r, const FootTables &T, const WordsPass &WP, bool read, bool match, bool decode, bool split, bool lattice, bool lmatch, bool ltrack, bool track, bool tdecode,
               bool ltdecode, const std::vector<uint32_t> &frame_of, const std::vector<int32_t> &frame_wh)
{
    const auto   t2 = std::chrono::steady_clock::now();
    const size_t n_lines = r->line_feet.size();
    if (const int rcw = words_collect(c, WP, n_lines, r->line_words, r->line_runs, r->words); rcw != STR_ER_OK) return rcw;
    r->have_line_words = true;
    if (read) {
        std::vector<double> slopes(n_lines);
        for (size_t t = 0; t < n_lines; ++t) slopes[t] = r->texts[t].slope;
        ReadChainOut out;          // (a consumer behind the scorer runs where its first table is given)
        out.words = &r->words; out.run_costs = &r->run_costs; out.run_probs = &r->run_probs;
        if (match) out.matches = &r->word_matches;
        if (decode) { out.decodes = &r->word_decodes; out.decode_chars = &r->word_decode_chars; out.decode_src = &r->word_decode_src; }
        const bool margin = decode && c->wd_margin;          // (a context setting, str_er_set_word_margin: no flag of its own)
        if (margin) { out.margins = &r->word_margins; out.row_margins = &r->word_row_margins; out.row_reads = &r->word_row_reads; out.row_alts = &r->word_row_alts; }
        const bool ldecode = decode && c->ln_on;          // (a context setting, str_er_set_line_decode: no flag of its own)
        if (ldecode) {
            out.line_decodes = &r->line_decodes; out.line_chars = &r->line_decode_chars; out.line_src = &r->line_decode_src; out.line_word_of_row = &r->line_decode_word_of_row;
            out.line_gaps = &r->line_gap_costs; out.line_windows = &r->line_decode_windows; out.n_lines = n_lines; out.line_bee = c->bigram_ee;
        }
        const bool lnmargin = ldecode && c->ln_margin;          // (a context setting, str_er_set_line_margin: no flag of its own)
        if (lnmargin) {
            out.line_margins = &r->line_margins; out.line_row_margins = &r->line_row_margins; out.line_row_reads = &r->line_row_reads; out.line_row_alts = &r->line_row_alts;
            out.line_gap_margins = &r->line_gap_margins; out.line_gap_moves = &r->line_gap_moves;
        }
        std::vector<uint8_t> piece_q;          // (the pieces' features are not part of the result)
        const RunPieces rp{&r->run_pieces, &r->piece_reads, &piece_q};
        if (split) {          // (the cut records of the compacted runs: down with the stage's wait)
            out.splits = &r->run_splits; out.piece_costs = &r->piece_costs; out.parts = &r->split_parts; out.word_splits = &r->word_splits;
            std::vector<uint32_t> slot_of(r->line_runs.size());
            for (size_t t = 0; t < n_lines; ++t)
                for (int32_t k = 0; k < r->line_words[t].n_runs; ++k) slot_of[(size_t)r->line_words[t].first_run + (size_t)k] = WP.slots[t].first + (uint32_t)k;
            if (const int rcs = run_cuts_collect(c, r->line_runs, slot_of, r->run_splits, r->run_pieces); rcs != STR_ER_OK) return rcs;
        }
        if (lattice && split) {
            out.lattice_decodes = &r->lattice_decodes; out.lattice_chars = &r->lattice_decode_chars; out.lattice_src = &r->lattice_decode_src; out.lattice_parts = &r->lattice_parts;
        }
        const bool lmargin = lattice && split && c->ld_margin;          // (a context setting, str_er_set_lattice_margin: no flag of its own)
        if (lmargin) {
            out.lattice_margins = &r->lattice_margins; out.lattice_read_margins = &r->lattice_read_margins; out.lattice_cut_margins = &r->lattice_cut_margins;
            out.lattice_part_reads = &r->lattice_part_reads; out.lattice_part_alts = &r->lattice_part_alts; out.lattice_cut_alts = &r->lattice_cut_alts;
        }
        const bool lldecode = lattice && split && c->ll_on;          // (a context setting, str_er_set_line_lattice_decode: no flag of its own)
        if (lldecode) {
            out.ll_decodes = &r->line_lattice_decodes; out.ll_chars = &r->line_lattice_chars; out.ll_src = &r->line_lattice_src; out.ll_parts = &r->line_lattice_parts;
            out.ll_word_of_part = &r->line_lattice_word_of_part; out.ll_gaps = &r->line_lattice_gap_costs; out.ll_windows = &r->line_lattice_windows;
            out.n_lines = n_lines; out.line_bee = c->bigram_ee;
        }
        if (lmatch && split && match) { out.lattice_matches = &r->lattice_matches; out.lattice_match_src = &r->lattice_match_src; out.lattice_match_parts = &r->lattice_match_parts; }
        if (track || tdecode) {
            out.tracks = &r->word_tracks; out.track_members = &r->word_track_members;
            if (track) { out.track_matches = &r->track_matches; out.track_member_costs = &r->track_member_costs; }
            if (tdecode) { out.track_decodes = &r->track_decodes; out.track_decode_chars = &r->track_decode_chars; out.track_decode_member_costs = &r->track_decode_member_costs; }
            if (!r->have_line_links || (track && !match) || (tdecode && !decode)) return fail(c, STR_ER_EHIP, "track read: no text tracks, no matcher or no decoder (internal error)");
            for (const str_er_line_word &w : r->words)
                if (w.line < 0 || (size_t)w.line >= n_lines || !str_er_tr::box_ok(w)) return fail(c, STR_ER_EHIP, "track read: a word outside the lines (internal error)");
            const auto           t3 = std::chrono::steady_clock::now();
            std::vector<uint8_t> reading(n_lines);
            str_er_tr::reading_lines(r->line_feet.data(), frame_of.data(), r->line_tracks.data(), (int32_t)n_lines, reading.data());
            str_er_tr::word_links(frame_of.data(), r->line_tracks.data(), reading.data(), (int32_t)n_lines, frame_wh.data(), r->words.data(), (int32_t)r->words.size(),
                                  c->wlink_num, c->wlink_den, r->word_links);
            str_er_tr::word_tracks(frame_of.data(), r->line_tracks.data(), reading.data(), r->words.data(), (int32_t)r->words.size(), r->word_links.data(),
                                   (int32_t)r->word_links.size(), r->word_track_of_words, r->word_tracks, r->word_track_members);
            for (const str_er_word_track &G : r->word_tracks)
                if (G.count > str_er_tr::MAX_MEMBERS) return fail(c, STR_ER_ECAPACITY, "STR_ER_WANT_TRACK_READ: a word track of more than 65536 members");
            for (const str_er_word_track &G : r->word_tracks)
                if (tdecode && G.count > str_er_td::MAX_MEMBERS) return fail(c, STR_ER_ECAPACITY, "STR_ER_WANT_TRACK_DECODE: a word track of more than 1024 members");
            if (c->dbg_stats)        // developer aid (tools/dev_track_read.py)
                std::fprintf(stderr, "[str_er] track read: %zu words, %zu word links, %zu word tracks, %zu members, host %.3f ms\n", r->words.size(), r->word_links.size(),
                             r->word_tracks.size(), r->word_track_members.size(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t3).count());
        }
        if (ltrack && track && lmatch && split && match) {
            out.lattice_track_matches = &r->lattice_track_matches; out.lattice_track_members = &r->lattice_track_members;
            out.lattice_track_src = &r->lattice_track_src; out.lattice_track_parts = &r->lattice_track_parts;
        }
        const bool ltd = ltdecode && tdecode && decode && lattice && split;          // (a context setting, str_er_set_lattice_track_decode: no flag of its own)
        if (ltd) {
            out.lattice_track_decodes = &r->lattice_track_decodes; out.lattice_track_decode_chars = &r->lattice_track_decode_chars;
            out.lattice_track_decode_members = &r->lattice_track_decode_members; out.lattice_track_decode_src = &r->lattice_track_decode_src;
            out.lattice_track_decode_parts = &r->lattice_track_decode_parts;
        }
        if (const int rcr = run_read_stage(c, s, T.lines, r->line_words, r->line_runs, slopes.data(), &r->run_reads, r->run_features, split ? &rp : nullptr, &out); rcr != STR_ER_OK)
            return rcr;
        r->have_track_read = track;
        r->have_word_tracks = track || tdecode;
        r->have_track_decodes = tdecode;
        r->have_lattice_track_decodes = ltd;
        r->have_run_splits = split;
        r->have_lattice_decodes = lattice && split;
        r->have_lattice_margins = lmargin;
        r->have_lattice_matches = lmatch && split && match;
        r->have_lattice_track = ltrack && track && lmatch && split && match;
        r->have_run_reads = true;
        r->have_word_matches = match;
        r->have_word_decodes = decode;
        r->have_word_margins = margin;
        r->have_line_decodes = ldecode;
        r->have_line_margins = lnmargin;
        r->have_line_lattice_decodes = lldecode;
    }
    if (c->dbg_stats)        // developer aid (tools/dev_line_words.py)
        std::fprintf(stderr, "[str_er] line words: %zu lines, %zu run slots reserved, %zu runs, %zu words, %zu bytes back, host %.3f ms\n", n_lines,
                     WP.n_elems, r->line_runs.size(), r->words.size(), WP.bytes_back(),
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count());
    return STR_ER_OK;
}

} // namespace

int frame_lines_phase(str_er_ctx *c, hipStream_t s, const Batch &b, float qscale, const uint32_t *d_mask_bits, const std::vector<uint64_t> *word_off,
                      str_er_result *r, const LineStageWants &want)
{
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n_frames = b.frame_wh.size() / 2, n_lines = r->texts.size();
    for (size_t f = 0; f < n_frames; ++f)
        if (b.frame_wh[2 * f] > 65535 || b.frame_wh[2 * f + 1] > 65535) return fail(c, STR_ER_ECAPACITY, "STR_ER_WANT_FRAME_LINES: a frame wider or taller than 65535 pixels");
    std::vector<uint32_t>   frame_of;
    std::vector<uint8_t>    pyr_of;
    std::vector<FootMember> mem;
    const uint32_t         *d_bits = nullptr;
    int rc = gather_members(c, s, b, qscale, d_mask_bits, word_off, r, frame_of, pyr_of, mem, d_bits);
    if (rc != STR_ER_OK) return rc;
    FootTables T;
    foot_layout(b.frame_wh, frame_of, mem, T, want.links);
    const double ms_layout = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    StageOut S(c);
    if (want.words && (rc = words_check_boxes(c, T.lines, "STR_ER_WANT_LINE_WORDS: ")) != STR_ER_OK) return rc;
    if ((rc = foot_stage(c, s, T, d_bits, true, want, S)) != STR_ER_OK) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    feet_from_stats(S.feet.stat, r->line_feet);
    if (want.geom)
        for (const str_er_line_foot &F : r->line_feet)
            if (F.w > GEOM_MAX_BOX || F.h > GEOM_MAX_BOX)
                return fail(c, STR_ER_ECAPACITY, "STR_ER_WANT_LINE_GEOM: a foot box wider or taller than " + std::to_string(GEOM_MAX_BOX) + " pixels");
    int32_t n_fl = 0;
    if ((rc = fill_frame_lines(c, r, frame_of, pyr_of, S.feet.pairs, n_fl)) != STR_ER_OK) return rc;
    if (want.links && (rc = fill_links(c, b, r, frame_of, T, S.links)) != STR_ER_OK) return rc;
    if (want.geom && (rc = fill_geometry(c, r, S.geom)) != STR_ER_OK) return rc;
    if (want.words && (rc = fill_words(c, s, r, T, S.words, want.read, want.match, want.decode, want.split, want.lattice, want.lmatch, want.ltrack, want.track, want.tdecode, want.ltdecode, frame_of, b.frame_wh)) != STR_ER_OK) return rc;
    if (c->dbg_stats)        // developer aid (tools/dev_frame_lines.py): the counts and the host side of the stage
        std::fprintf(stderr, "[str_er] frame lines: %zu lines, %zu members, %zu jobs, %llu footprint words, %u candidate pairs, %zu pairs, %d frame lines, "
                             "%zu bytes back, host %.3f ms before + %.3f ms after the device\n",
                     n_lines, T.members.size(), T.jobs.size(), (unsigned long long)T.words, S.feet.n_candidates, S.feet.pairs.size(), n_fl, S.feet.bytes_back, ms_layout,
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
    return STR_ER_OK;
}

int feet_words_read(str_er_ctx *c, int32_t W, int32_t H, const str_er_line_foot *feet, const uint32_t *bits, int32_t n, str_er_line_words *line_words,
                    str_er_line_run *runs, int32_t cap_runs, int32_t *n_runs, str_er_line_word *words, int32_t cap_words, int32_t *n_words, bool read_runs,
                    const double *slopes, str_er_run_read *reads, uint8_t *q_out, const FeetSplitOut *split)
{
    if (split && (!split->splits || !split->n_pieces || (split->pieces && split->cap_pieces < 0))) return fail(c, STR_ER_EINVAL, "bad arguments");
    if (W < 1 || H < 1 || W > 65535 || H > 65535 || n < 0 || !n_runs || !n_words || (n > 0 && (!feet || !line_words)) || (runs && cap_runs < 0) ||
        (words && cap_words < 0))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    if (split) *split->n_pieces = 0;
    CallerFeet F(c);
    int rc = F.check_boxes(W, H, feet, n, "");
    if (rc != STR_ER_OK) return rc;
    const bool reading = read_runs && runs && words;          // (a counting call reads nothing)
    const bool scoring = reads || (split && split->pieces && split->piece_reads);
    if (read_runs && scoring && !(c->svm_loaded && c->svm.dim == 1800))
        return fail(c, STR_ER_ESTATE, std::string(split ? "str_er_feet_split" : "str_er_feet_read") + " needs an SVM model loaded with dim = 1800 (str_er_load_svm_model)");
    if (read_runs && slopes)
        for (int32_t t = 0; t < n; ++t)
            if (!std::isfinite(slopes[t])) return fail(c, STR_ER_EINVAL, "slope " + std::to_string(t) + " is not finite");
    if ((rc = F.check_limit(feet, n, WORDS_MAX_BOX)) != STR_ER_OK || (rc = F.pack(feet, bits, n, true)) != STR_ER_OK) return rc;
    WordsPass WP = words_pass(c);
    if (!F.words.empty()) {
        const size_t tab_need = sizeof(FootLine) * (size_t)n;
        if ((rc = F.reserve(tab_need)) != STR_ER_OK || (rc = F.upload(tab_need)) != STR_ER_OK) return rc;
        if ((rc = words_enqueue(c, c->stream, F.lines, F.d_lines(), WP)) != STR_ER_OK) return rc;
        // (the cuts ride on the same wait: k_run_cuts reads the run slots where k_foot_words left them)
        if (split && reading && (rc = run_cuts_enqueue(c, c->stream, F.d_lines(), n, WP.buf.d(), WP.o_rec, WP.o_elem, WP.n_elems)) != STR_ER_OK) return rc;
        if ((rc = F.wait()) != STR_ER_OK) return rc;
    }
    std::vector<str_er_line_words> lw;
    std::vector<str_er_line_run>   rn;
    std::vector<str_er_line_word>  wd;
    if ((rc = words_collect(c, WP, (size_t)n, lw, rn, wd)) != STR_ER_OK) return rc;
    *n_runs = (int32_t)rn.size(); *n_words = (int32_t)wd.size();
    if (n > 0) std::memcpy(line_words, lw.data(), sizeof(str_er_line_words) * (size_t)n);
    if (!runs || !words) return STR_ER_OK;
    if ((rc = check_cap(c, rn.size(), cap_runs, "glyph runs, cap_runs")) != STR_ER_OK || (rc = check_cap(c, wd.size(), cap_words, "words, cap_words")) != STR_ER_OK)
        return rc;
    std::vector<str_er_run_split> sp;
    std::vector<str_er_run_piece> pc;
    if (split && reading && !rn.empty()) {
        std::vector<uint32_t> slot_of(rn.size());
        for (size_t t = 0; t < (size_t)n; ++t)
            for (int32_t k = 0; k < lw[t].n_runs; ++k) slot_of[(size_t)lw[t].first_run + (size_t)k] = WP.slots[t].first + (uint32_t)k;
        if ((rc = run_cuts_collect(c, rn, slot_of, sp, pc)) != STR_ER_OK) return rc;
        *split->n_pieces = (int32_t)pc.size();
        if (split->pieces && (rc = check_cap(c, pc.size(), split->cap_pieces, "pieces, cap_pieces")) != STR_ER_OK) return rc;
    }
    const bool with_pieces = split && split->pieces;
    if (reading && !rn.empty()) {          // (the footprints are still in c->foot_bits, the lines as the kernel read them in F.lines)
        std::vector<str_er_run_read> rd, prd;
        std::vector<uint8_t>         q, pq;
        const RunPieces RP{&pc, split && split->piece_reads ? &prd : nullptr, &pq};
        if ((rc = run_read_stage(c, c->stream, F.lines, lw, rn, slopes, scoring ? &rd : nullptr, q, with_pieces ? &RP : nullptr)) != STR_ER_OK)
            return rc;
        if (reads) std::memcpy(reads, rd.data(), sizeof(str_er_run_read) * rd.size());
        if (q_out) std::memcpy(q_out, q.data(), q.size());
        if (with_pieces && split->piece_reads && !prd.empty()) std::memcpy(split->piece_reads, prd.data(), sizeof(str_er_run_read) * prd.size());
        if (with_pieces && split->piece_q && !pq.empty()) std::memcpy(split->piece_q, pq.data(), pq.size());
    }
    if (split && !sp.empty()) std::memcpy(split->splits, sp.data(), sizeof(str_er_run_split) * sp.size());
    if (with_pieces && !pc.empty()) std::memcpy(split->pieces, pc.data(), sizeof(str_er_run_piece) * pc.size());
    if (!rn.empty()) std::memcpy(runs, rn.data(), sizeof(str_er_line_run) * rn.size());
    if (!wd.empty()) std::memcpy(words, wd.data(), sizeof(str_er_line_word) * wd.size());
    return STR_ER_OK;
}

} // namespace str_er_host

extern "C" {

int str_er_set_frame_merge(str_er_ctx *c, int32_t num, int32_t den)
{
    if (!c) return STR_ER_EINVAL;
    if (num < 1 || num > den || den > 65535) return fail(c, STR_ER_EINVAL, "str_er_set_frame_merge: 1 <= num <= den <= 65535");
    c->merge_num = num; c->merge_den = den;
    return STR_ER_OK;
}

int str_er_line_feet_regions(str_er_ctx *c, const uint8_t *plane, int32_t w, int32_t h, int64_t stride, const str_er_cand *regions,
                             const int32_t *line_of, int32_t n, int32_t n_lines, int32_t out_w, int32_t out_h, str_er_line_foot *feet,
                             uint32_t *bits, uint64_t cap_words, uint64_t *n_words, str_er_line_pair *pairs, int32_t cap_pairs,
                             int32_t *n_pairs)
try {
    if (!c) return STR_ER_EINVAL;
    if (out_w < 1 || out_h < 1 || n_lines < 0 || !n_words || !n_pairs || (n_lines > 0 && !feet) || (n > 0 && !line_of) || (pairs && cap_pairs < 0))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    if (out_w > 65535 || out_h > 65535) return fail(c, STR_ER_ECAPACITY, "line feet: an output wider or taller than 65535 pixels");
    const DetectParams dp = make_dp(c);
    std::vector<MaskJob> jobs;
    uint64_t words = 0;
    int rc = region_jobs(c, plane, w, h, stride, regions, n, dp, jobs, words);
    if (rc != STR_ER_OK) return rc;
    for (int32_t i = 0; i < n; ++i)
        if (line_of[i] < 0 || line_of[i] >= n_lines) return fail(c, STR_ER_EINVAL, "region " + std::to_string(i) + ": line outside [0, n_lines)");
    HIP_TRY(c, hipSetDevice(c->prm.device));
    // the members by line (the regions of a line in their order)
    std::vector<int32_t> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t p, int32_t q) { return line_of[p] < line_of[q]; });
    std::vector<FootMember> mem((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        const str_er_cand &g = regions[order[(size_t)i]];
        FootMember &m = mem[(size_t)i];
        m.line = (uint32_t)line_of[order[(size_t)i]]; m.pw = w; m.ph = h; m.x = g.x; m.y = g.y; m.w = g.w; m.h = g.h;
        m.word_off = jobs[(size_t)order[(size_t)i]].out_off;
    }
    const uint32_t *d_bits = nullptr;
    if (n > 0) {
        if ((rc = region_upload(c, plane, w, h, stride, jobs)) != STR_ER_OK) return rc;
        if ((rc = mask_launch(c, c->stream, jobs, words, dp.qscale, &d_bits)) != STR_ER_OK) return rc;
    }
    const std::vector<int32_t>  frame_wh = {out_w, out_h};
    const std::vector<uint32_t> frame_of((size_t)n_lines, 0);
    const std::vector<uint8_t>  pyr_of((size_t)n_lines, 0);
    FootTables T;
    foot_layout(frame_wh, frame_of, mem, T);
    StageOut S(c);
    if ((rc = foot_stage(c, c->stream, T, d_bits, false, LineStageWants{}, S)) != STR_ER_OK) return rc;
    const FootOut &O = S.feet;
    std::vector<str_er_line_foot> ft;
    feet_from_stats(O.stat, ft);
    std::vector<str_er_line_pair> pr(O.pairs.size());
    if (!pr.empty()) std::memcpy(pr.data(), O.pairs.data(), sizeof(FootPair) * pr.size());
    int32_t n_fl = 0;
    if (str_er_frame_lines_from_pairs(ft.data(), frame_of.data(), pyr_of.data(), n_lines, pr.data(), (int32_t)pr.size(), c->merge_num, c->merge_den, nullptr, 0,
                                      &n_fl, nullptr) != STR_ER_OK)
        return fail(c, STR_ER_EHIP, "line feet: the device's pairs do not fit its footprints (internal error)");
    uint64_t out_words = 0;
    for (const str_er_line_foot &F : ft) out_words += (uint64_t)F.h * (((uint32_t)F.w + 31u) / 32u);
    *n_words = out_words;
    *n_pairs = (int32_t)pr.size();
    if (n_lines > 0) std::memcpy(feet, ft.data(), sizeof(str_er_line_foot) * (size_t)n_lines);
    if (bits && out_words > cap_words)
        return fail(c, STR_ER_ECAPACITY, "the footprints need " + std::to_string(out_words) + " words, cap_words is " + std::to_string(cap_words));
    if ((rc = copy_out(c, pr.data(), pr.size(), sizeof(str_er_line_pair), pairs, cap_pairs, "pairs, cap_pairs")) != STR_ER_OK) return rc;
    if (bits && out_words) {
        // the footprints back as they lie on the device (64-bit words over the union of the pre-image boxes), cut to the foot boxes
        std::vector<uint64_t> dev((size_t)T.words);
        HIP_TRY(c, hipMemcpy(dev.data(), c->foot_bits.d<uint64_t>(), 8 * (size_t)T.words, hipMemcpyDeviceToHost));
        std::vector<uint32_t> cut;
        cut.reserve((size_t)out_words);
        for (int32_t t = 0; t < n_lines; ++t) foot_rows32(dev.data() + T.lines[(size_t)t].word_off, T.lines[(size_t)t], ft[(size_t)t], cut);
        std::memcpy(bits, cut.data(), 4 * cut.size());
    }
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_set_line_link(str_er_ctx *c, int32_t num, int32_t den)
{
    if (!c) return STR_ER_EINVAL;
    if (num < 1 || num > den || den > 65535) return fail(c, STR_ER_EINVAL, "str_er_set_line_link: 1 <= num <= den <= 65535");
    c->link_num = num; c->link_den = den;
    return STR_ER_OK;
}

int str_er_link_feet(str_er_ctx *c, int32_t W, int32_t H, const str_er_line_foot *feet_a, const uint32_t *bits_a, int32_t n_a,
                     const str_er_line_foot *feet_b, const uint32_t *bits_b, int32_t n_b, str_er_line_link *pairs, int32_t cap_pairs, int32_t *n_pairs)
try {
    if (!c) return STR_ER_EINVAL;
    if (W < 1 || H < 1 || W > 65535 || H > 65535 || n_a < 0 || n_b < 0 || !n_pairs || (n_a > 0 && !feet_a) || (n_b > 0 && !feet_b) || (pairs && cap_pairs < 0))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    // the two sets as one table of lines, a's first
    const size_t n_lines = (size_t)n_a + (size_t)n_b;
    CallerFeet F(c);
    int rc = F.check_boxes(W, H, feet_a, n_a, "set a, ");
    if (rc != STR_ER_OK || (rc = F.check_boxes(W, H, feet_b, n_b, "set b, ")) != STR_ER_OK) return rc;
    if ((rc = F.pack(feet_a, bits_a, n_a, false)) != STR_ER_OK || (rc = F.pack(feet_b, bits_b, n_b, false)) != STR_ER_OK) return rc;
    *n_pairs = 0;
    if (n_a == 0 || n_b == 0 || F.words.empty()) return STR_ER_OK;
    std::vector<FootRange> range(n_lines, FootRange{0, 0});
    std::vector<uint32_t>  list((size_t)n_b);
    for (int32_t i = 0; i < n_a; ++i) range[(size_t)i] = FootRange{0, (uint32_t)n_b};
    std::iota(list.begin(), list.end(), (uint32_t)n_a);
    const size_t o_list = align_up(sizeof(FootLine) * n_lines, 256), o_rng = align_up(o_list + 4 * list.size(), 256), tab_need = o_rng + sizeof(FootRange) * n_lines;
    PairTable LT = link_table(c);
    if ((rc = F.reserve(tab_need)) != STR_ER_OK || (rc = LT.reserve(c, n_lines)) != STR_ER_OK) return rc;
    std::memcpy(c->foot_tab.h() + o_list, list.data(), 4 * list.size());
    std::memcpy(c->foot_tab.h() + o_rng, range.data(), sizeof(FootRange) * n_lines);
    if ((rc = F.upload(tab_need)) != STR_ER_OK) return rc;
    hipStream_t s = c->stream;
    const auto launch = [&](FootHead *head, FootPair *out, uint32_t cap) {
        launch_foot_links(s, F.d_lines(), (int)n_lines, reinterpret_cast<const FootRange *>(c->foot_tab.d() + o_rng),
                          reinterpret_cast<const uint32_t *>(c->foot_tab.d() + o_list), c->foot_bits.d<uint64_t>(), head, out, cap);
    };
    std::vector<FootPair> got;
    for (bool again = true; again;) {
        if ((rc = LT.enqueue(c, s, launch)) != STR_ER_OK || (rc = F.wait()) != STR_ER_OK) return rc;
        if ((rc = LT.collect(c, got, again)) != STR_ER_OK) return rc;
    }
    sort_pairs(got);
    *n_pairs = (int32_t)got.size();
    if (pairs)          // the records as the caller's (str_er_line_link): b within its set, and the link
        for (FootPair &P : got) {
            P.b -= n_a;
            P.dup = overlap_passes(P.inter, feet_a[P.a].pixels, feet_b[P.b].pixels, c->link_num, c->link_den) ? 1u : 0u;
        }
    return copy_out(c, got.data(), got.size(), sizeof(FootPair), pairs, cap_pairs, "pairs, cap_pairs");
} ABI_GUARD(c)

int str_er_feet_geom(str_er_ctx *c, int32_t W, int32_t H, const str_er_line_foot *feet, const uint32_t *bits, int32_t n, str_er_line_geom *geoms, int32_t *xy,
                     int32_t cap_points, int32_t *n_points)
try {
    if (!c) return STR_ER_EINVAL;
    if (W < 1 || H < 1 || W > 65535 || H > 65535 || n < 0 || !n_points || (n > 0 && (!feet || !geoms)) || (xy && cap_points < 0))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    CallerFeet F(c);
    int rc = F.check_boxes(W, H, feet, n, "");
    if (rc != STR_ER_OK || (rc = F.check_limit(feet, n, GEOM_MAX_BOX)) != STR_ER_OK || (rc = F.pack(feet, bits, n, true)) != STR_ER_OK) return rc;
    GeomPass GP = geom_pass(c);
    if (!F.words.empty()) {
        const size_t tab_need = sizeof(FootLine) * (size_t)n;
        if ((rc = F.reserve(tab_need)) != STR_ER_OK || (rc = F.upload(tab_need)) != STR_ER_OK) return rc;
        if ((rc = geom_enqueue(c, c->stream, F.lines, F.d_lines(), GP)) != STR_ER_OK || (rc = F.wait()) != STR_ER_OK) return rc;
    }
    std::vector<str_er_line_geom> out;
    std::vector<int32_t>          pts;
    if ((rc = geom_collect(c, GP, (size_t)n, out, pts)) != STR_ER_OK) return rc;
    *n_points = (int32_t)(pts.size() / 2);
    if (n > 0) std::memcpy(geoms, out.data(), sizeof(str_er_line_geom) * (size_t)n);
    return copy_out(c, pts.data(), pts.size() / 2, 8, xy, cap_points, "hull vertices, cap_points");
} ABI_GUARD(c)

int str_er_set_word_gap(str_er_ctx *c, int32_t num, int32_t den)
{
    if (!c) return STR_ER_EINVAL;
    if (!word_gap_ok(num, den)) return fail(c, STR_ER_EINVAL, "str_er_set_word_gap: 1 <= num, den <= 65535");
    c->word_num = num; c->word_den = den;
    return STR_ER_OK;
}

int str_er_feet_words(str_er_ctx *c, int32_t W, int32_t H, const str_er_line_foot *feet, const uint32_t *bits, int32_t n, str_er_line_words *line_words,
                      str_er_line_run *runs, int32_t cap_runs, int32_t *n_runs, str_er_line_word *words, int32_t cap_words, int32_t *n_words)
try {
    if (!c) return STR_ER_EINVAL;
    return feet_words_read(c, W, H, feet, bits, n, line_words, runs, cap_runs, n_runs, words, cap_words, n_words, false, nullptr, nullptr, nullptr);
} ABI_GUARD(c)

const str_er_run_read *str_er_result_run_reads(const str_er_result *r, int32_t *n) { return result_table(r, r && r->have_run_reads, &str_er_result::run_reads, n); }

const uint8_t *str_er_result_run_features(const str_er_result *r, uint64_t *n_bytes) { return result_table(r, r && r->have_run_reads, &str_er_result::run_features, n_bytes); }

const str_er_line_words *str_er_result_line_words(const str_er_result *r, int32_t *n) { return result_table(r, r && r->have_line_words, &str_er_result::line_words, n); }

const str_er_line_run *str_er_result_line_runs(const str_er_result *r, int32_t *n) { return result_table(r, r && r->have_line_words, &str_er_result::line_runs, n); }

const str_er_line_word *str_er_result_words(const str_er_result *r, int32_t *n) { return result_table(r, r && r->have_line_words, &str_er_result::words, n); }

const str_er_line_geom *str_er_result_line_geoms(const str_er_result *r, int32_t *n) { return result_table(r, r && r->have_line_geom, &str_er_result::line_geoms, n); }

const str_er_line_geom *str_er_result_frame_line_geoms(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_line_geom, &str_er_result::frame_line_geoms, n);
}

const int32_t *str_er_result_geom_points(const str_er_result *r, int32_t *n_points)
{
    int32_t n2 = 0;
    const int32_t *p = result_table(r, r && r->have_line_geom, &str_er_result::geom_points, &n2);
    if (n_points) *n_points = n2 / 2;
    return p;
}

const str_er_line_link *str_er_result_line_links(const str_er_result *r, int32_t *n) { return result_table(r, r && r->have_line_links, &str_er_result::line_links, n); }

const int32_t *str_er_result_line_tracks(const str_er_result *r, int32_t *n) { return result_table(r, r && r->have_line_links, &str_er_result::line_tracks, n); }

const str_er_text_track *str_er_result_text_tracks(const str_er_result *r, int32_t *n) { return result_table(r, r && r->have_line_links, &str_er_result::text_tracks, n); }

const int32_t *str_er_result_text_track_members(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_line_links, &str_er_result::text_track_members, n);
}

int str_er_result_edge_feet(const str_er_result *r, int32_t which, int32_t *frame_w, int32_t *frame_h, const str_er_line_foot **feet, const int32_t **lines,
                            int32_t *n, const uint32_t **bits, uint64_t *n_words)
{
    static const str_er_line_foot no_foot{};
    static const int32_t  no_line = 0;
    static const uint32_t no_bits = 0;
    if (!r || !r->have_line_links || which < 0 || which > 1) return STR_ER_EINVAL;
    const str_er_result::EdgeFeet &E = r->edge_feet[which];
    if (frame_w) *frame_w = E.w;
    if (frame_h) *frame_h = E.h;
    if (feet) *feet = E.feet.empty() ? &no_foot : E.feet.data();
    if (lines) *lines = E.lines.empty() ? &no_line : E.lines.data();
    if (n) *n = (int32_t)E.feet.size();
    if (bits) *bits = E.bits.empty() ? &no_bits : E.bits.data();
    if (n_words) *n_words = E.bits.size();
    return STR_ER_OK;
}

const str_er_line_foot *str_er_result_line_feet(const str_er_result *r, int32_t *n) { return result_table(r, r && r->have_frame_lines, &str_er_result::line_feet, n); }

const str_er_line_pair *str_er_result_line_pairs(const str_er_result *r, int32_t *n) { return result_table(r, r && r->have_frame_lines, &str_er_result::line_pairs, n); }

const str_er_frame_line *str_er_result_frame_lines(const str_er_result *r, int32_t *n) { return result_table(r, r && r->have_frame_lines, &str_er_result::frame_lines, n); }

const int32_t *str_er_result_frame_line_members(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_frame_lines, &str_er_result::frame_line_members, n);
}

} // extern "C"
