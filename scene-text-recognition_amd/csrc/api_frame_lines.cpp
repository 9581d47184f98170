// api_frame_lines.cpp -- the C ABI, part 8: one list of text lines per frame, merged across pyramid levels (STR_ER_WANT_FRAME_LINES in
// run_batch, str_er_line_feet_regions on one host plane, str_er_frame_lines_from_pairs on the host alone) and the result accessors.
// The contract is at str_er_line_foot (str_er.h).  The host lists the members of every line with their pre-image boxes, cuts the
// footprints into jobs and lists the lines of every frame; k_line_foot and k_foot_pairs (er_frame_lines.inl) do the per-pixel work;
// the host sorts the pairs that come back and joins the duplicates (union-find).
#include "str_er_ctx.h"

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
};

constexpr uint32_t FOOT_JOB_WORDS = 1024;        // 64-bit words of a job of k_line_foot: 16 per lane

// members: ordered by line; frame_of[t]: the frame of line t, frame_wh its level-0 size
void foot_layout(const std::vector<int32_t> &frame_wh, const std::vector<uint32_t> &frame_of, const std::vector<FootMember> &mem, FootTables &T)
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
}

struct FootOut {
    std::vector<FootStat> stat;          // per line
    std::vector<FootPair> pairs;         // inter > 0, sorted by (a, b)
    uint32_t n_candidates = 0;
    size_t   bytes_back = 0;
};

// one upload, the two launches on s, one copy back, one wait (the pair pass again, with a larger table, if the pairs outgrew it)
int foot_stage(str_er_ctx *c, hipStream_t s, const FootTables &T, const uint32_t *d_bits, bool in_batch, FootOut &O)
{
    const size_t n_lines = T.lines.size();
    O.stat.assign(n_lines, FootStat{});
    O.pairs.clear();
    if (T.members.empty()) return STR_ER_OK;
    const size_t o_jobs = align_up(sizeof(FootLine) * n_lines, 256), o_list = align_up(o_jobs + sizeof(FootJob) * T.jobs.size(), 256);
    const size_t o_mem = align_up(o_list + 4 * T.list.size(), 256), o_tab = align_up(o_mem + sizeof(TextMapCand) * T.members.size(), 256);
    const size_t tab_need = o_tab + 2 * T.st.tabs.size();
    int rc = grow_pair(c, c->d_foot_tab, c->h_foot_tab, c->foot_tab_bytes, tab_need, "frame line tables");
    if (rc != STR_ER_OK) return rc;
    if (T.words > c->foot_bits_words) {
        const size_t get = std::max<size_t>((size_t)T.words, 2 * c->foot_bits_words);
        if (c->d_foot_bits) { (void)hipFree(c->d_foot_bits); c->d_foot_bits = nullptr; }
        c->foot_bits_words = 0;
        if (hipMalloc(reinterpret_cast<void **>(&c->d_foot_bits), 8 * get) != hipSuccess)
            return fail(c, STR_ER_ENOMEM, "hipMalloc (line footprints, " + std::to_string(8 * get) + " bytes)");
        c->foot_bits_words = get;
    }
    const size_t o_stat = sizeof(FootHead), o_pairs = o_stat + sizeof(FootStat) * n_lines;
    size_t cap = std::max<size_t>(1024, 4 * n_lines);
    if (c->foot_out_bytes > o_pairs) cap = std::max(cap, (c->foot_out_bytes - o_pairs) / sizeof(FootPair));
    if ((rc = grow_pair(c, c->d_foot_out, c->h_foot_out, c->foot_out_bytes, o_pairs + sizeof(FootPair) * cap, "frame line output")) != STR_ER_OK) return rc;
    std::memcpy(c->h_foot_tab, T.lines.data(), sizeof(FootLine) * n_lines);
    if (!T.jobs.empty()) std::memcpy(c->h_foot_tab + o_jobs, T.jobs.data(), sizeof(FootJob) * T.jobs.size());
    std::memcpy(c->h_foot_tab + o_list, T.list.data(), 4 * T.list.size());
    std::memcpy(c->h_foot_tab + o_mem, T.members.data(), sizeof(TextMapCand) * T.members.size());
    std::memcpy(c->h_foot_tab + o_tab, T.st.tabs.data(), 2 * T.st.tabs.size());
    HIP_TRY(c, hipMemcpyAsync(c->d_foot_tab, c->h_foot_tab, tab_need, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(c->d_foot_out, 0, o_pairs, s));
    const FootLine *d_lines = reinterpret_cast<const FootLine *>(c->d_foot_tab);
    const uint32_t *d_list = reinterpret_cast<const uint32_t *>(c->d_foot_tab + o_list);
    launch_line_foot(s, reinterpret_cast<const FootJob *>(c->d_foot_tab + o_jobs), (int)T.jobs.size(), d_lines,
                     reinterpret_cast<const TextMapCand *>(c->d_foot_tab + o_mem), reinterpret_cast<const uint16_t *>(c->d_foot_tab + o_tab), d_bits,
                     c->d_foot_bits, reinterpret_cast<FootStat *>(c->d_foot_out + o_stat));
    HIP_TRY(c, hipGetLastError());
    for (int pass = 0;; ++pass) {
        launch_foot_pairs(s, d_lines, (int)n_lines, d_list, c->d_foot_bits, reinterpret_cast<FootHead *>(c->d_foot_out),
                          reinterpret_cast<FootPair *>(c->d_foot_out + o_pairs), (uint32_t)cap);
        HIP_TRY(c, hipGetLastError());
        if (in_batch && pass == 0) rec(c, "frame_lines");          // (the call's one profiling event of the stage)
        // what comes back: the counters, the statistics and the pairs in one copy (the table is sized for four pairs a line: all of it is a
        // few hundred KB at most for a batch; the host reads as many as the counter says)
        const size_t back = o_pairs + sizeof(FootPair) * cap;
        HIP_TRY(c, hipMemcpyAsync(c->h_foot_out, c->d_foot_out, back, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, wait_stream(c, s));
        O.bytes_back += back;
        FootHead head;
        std::memcpy(&head, c->h_foot_out, sizeof head);
        if (pass == 0) std::memcpy(O.stat.data(), c->h_foot_out + o_stat, sizeof(FootStat) * n_lines);
        O.n_candidates = head.n_candidates;
        if (head.n_pairs <= cap) {
            O.pairs.resize(head.n_pairs);
            if (head.n_pairs) std::memcpy(O.pairs.data(), c->h_foot_out + o_pairs, sizeof(FootPair) * head.n_pairs);
            break;
        }
        if (pass > 0) return fail(c, STR_ER_EHIP, "frame lines: the pair table overflowed twice (internal error)");
        // more pairs than the table holds: a table for all of them, and the pair pass once more (the footprints are still on the device)
        cap = head.n_pairs;
        if ((rc = grow_pair(c, c->d_foot_out, c->h_foot_out, c->foot_out_bytes, o_pairs + sizeof(FootPair) * cap, "frame line output")) != STR_ER_OK) return rc;
        HIP_TRY(c, hipMemsetAsync(c->d_foot_out, 0, o_pairs, s));
    }
    std::sort(O.pairs.begin(), O.pairs.end(), [](const FootPair &p, const FootPair &q) { return p.a != q.a ? p.a < q.a : p.b < q.b; });
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

int find_root(std::vector<int32_t> &parent, int32_t t)
{
    while (parent[(size_t)t] != t) { parent[(size_t)t] = parent[(size_t)parent[(size_t)t]]; t = parent[(size_t)t]; }
    return t;
}

static_assert(sizeof(FootPair) == sizeof(str_er_line_pair), "the device writes str_er_line_pair records");

} // namespace

int frame_lines_phase(str_er_ctx *c, hipStream_t s, const Batch &b, float qscale, const uint32_t *d_mask_bits, const std::vector<uint64_t> *word_off,
                      str_er_result *r)
{
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n_frames = b.frame_wh.size() / 2, n_lines = r->texts.size();
    for (size_t f = 0; f < n_frames; ++f)
        if (b.frame_wh[2 * f] > 65535 || b.frame_wh[2 * f + 1] > 65535) return fail(c, STR_ER_ECAPACITY, "STR_ER_WANT_FRAME_LINES: a frame wider or taller than 65535 pixels");
    // the members of every line, each once
    std::vector<uint32_t> frame_of(n_lines);
    std::vector<uint8_t>  pyr_of(n_lines);
    std::vector<FootMember> mem;
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
    const uint32_t *d_bits = d_mask_bits;
    if (d_mask_bits && word_off) {
        for (size_t i = 0; i < mem.size(); ++i) {
            mem[i].word_off = (*word_off)[who[i]];
            if (mem[i].word_off == UINT64_MAX) return fail(c, STR_ER_EHIP, "frame lines: a member without a mask (internal error)");
        }
    } else if (!mem.empty()) {
        // the masks of the candidates that are members, made by the mask kernels and left on the device
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
    FootTables T;
    foot_layout(b.frame_wh, frame_of, mem, T);
    const double ms_layout = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    FootOut O;
    const int rc = foot_stage(c, s, T, d_bits, true, O);
    if (rc != STR_ER_OK) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    feet_from_stats(O.stat, r->line_feet);
    r->line_pairs.resize(O.pairs.size());
    if (!O.pairs.empty()) std::memcpy(r->line_pairs.data(), O.pairs.data(), sizeof(FootPair) * O.pairs.size());
    r->frame_lines.resize(n_lines);
    r->frame_line_members.resize(n_lines);
    int32_t n_fl = 0;
    const int rcf = str_er_frame_lines_from_pairs(r->line_feet.data(), frame_of.data(), pyr_of.data(), (int32_t)n_lines, r->line_pairs.data(),
                                                  (int32_t)r->line_pairs.size(), c->merge_num, c->merge_den, r->frame_lines.data(), (int32_t)n_lines, &n_fl,
                                                  r->frame_line_members.data());
    if (rcf != STR_ER_OK) return fail(c, STR_ER_EHIP, "frame lines: the device's pairs do not fit its footprints (internal error)");
    r->frame_lines.resize((size_t)n_fl);
    r->have_frame_lines = true;
    if (c->dbg_stats)        // developer aid (tools/dev_frame_lines.py): the counts and the host side of the stage
        std::fprintf(stderr, "[str_er] frame lines: %zu lines, %zu members, %zu jobs, %llu footprint words, %u candidate pairs, %zu pairs, %d frame lines, "
                             "%zu bytes back, host %.3f ms before + %.3f ms after the device\n",
                     n_lines, T.members.size(), T.jobs.size(), (unsigned long long)T.words, O.n_candidates, O.pairs.size(), n_fl, O.bytes_back, ms_layout,
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
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

int str_er_frame_lines_from_pairs(str_er_line_foot *feet, const uint32_t *frames_of_lines, const uint8_t *pyr_of_lines, int32_t n_lines,
                                  str_er_line_pair *pairs, int32_t n_pairs, int32_t num, int32_t den, str_er_frame_line *frame_lines,
                                  int32_t cap_frame_lines, int32_t *n_frame_lines, int32_t *members)
try {
    if (n_lines < 0 || n_pairs < 0 || !n_frame_lines || num < 1 || num > den || den > 65535) return STR_ER_EINVAL;
    if (n_lines > 0 && (!feet || !frames_of_lines || !pyr_of_lines)) return STR_ER_EINVAL;
    if ((n_pairs > 0 && !pairs) || (frame_lines && n_lines > 0 && !members) || (frame_lines && cap_frame_lines < 0)) return STR_ER_EINVAL;
    for (int32_t k = 0; k < n_pairs; ++k) {
        const str_er_line_pair &P = pairs[k];
        if (P.a < 0 || P.a >= P.b || P.b >= n_lines || frames_of_lines[P.a] != frames_of_lines[P.b]) return STR_ER_EINVAL;
        if (P.inter == 0 || P.inter > feet[P.a].pixels || P.inter > feet[P.b].pixels) return STR_ER_EINVAL;
    }
    // the duplicates joined: the root of a component is its smallest line
    std::vector<int32_t> parent((size_t)n_lines);
    std::iota(parent.begin(), parent.end(), 0);
    for (int32_t k = 0; k < n_pairs; ++k) {
        str_er_line_pair &P = pairs[k];
        const uint64_t uni = (uint64_t)feet[P.a].pixels + (uint64_t)feet[P.b].pixels - (uint64_t)P.inter;
        P.dup = (uint64_t)P.inter * (uint64_t)den >= (uint64_t)num * uni ? 1u : 0u;
        if (!P.dup) continue;
        const int32_t ra = find_root(parent, P.a), rb = find_root(parent, P.b);
        if (ra != rb) parent[(size_t)std::max(ra, rb)] = std::min(ra, rb);
    }
    // the frame lines: by frame, then by smallest member
    std::vector<int32_t> roots;
    for (int32_t t = 0; t < n_lines; ++t)
        if (find_root(parent, t) == t) roots.push_back(t);
    std::sort(roots.begin(), roots.end(), [&](int32_t p, int32_t q) { return frames_of_lines[p] != frames_of_lines[q] ? frames_of_lines[p] < frames_of_lines[q] : p < q; });
    std::vector<int32_t> index_of((size_t)n_lines, -1);
    for (size_t i = 0; i < roots.size(); ++i) index_of[(size_t)roots[i]] = (int32_t)i;
    for (int32_t t = 0; t < n_lines; ++t) feet[t].frame_line = index_of[(size_t)find_root(parent, t)];
    *n_frame_lines = (int32_t)roots.size();
    if (!frame_lines) return STR_ER_OK;
    if ((int32_t)roots.size() > cap_frame_lines) return STR_ER_ECAPACITY;
    for (size_t i = 0; i < roots.size(); ++i) {
        str_er_frame_line &G = frame_lines[i];
        G = str_er_frame_line{};
        G.frame = frames_of_lines[roots[i]]; G.rep = -1;
    }
    for (int32_t t = 0; t < n_lines; ++t) ++frame_lines[feet[t].frame_line].count;
    int32_t at = 0;
    for (size_t i = 0; i < roots.size(); ++i) { frame_lines[i].first = at; at += frame_lines[i].count; frame_lines[i].count = 0; }
    for (int32_t t = 0; t < n_lines; ++t) {          // (ascending t: the members ascend, and a tie of pixels stays with the smaller line)
        str_er_frame_line      &G = frame_lines[feet[t].frame_line];
        const str_er_line_foot &F = feet[t];
        members[G.first + G.count++] = t;
        if (G.rep < 0 || F.pixels > G.pixels) { G.rep = t; G.pixels = F.pixels; }
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
    FootOut O;
    if ((rc = foot_stage(c, c->stream, T, d_bits, false, O)) != STR_ER_OK) return rc;
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
    if (pairs && (int64_t)pr.size() > (int64_t)cap_pairs)
        return fail(c, STR_ER_ECAPACITY, std::to_string(pr.size()) + " pairs, cap_pairs is " + std::to_string(cap_pairs));
    if (pairs && !pr.empty()) std::memcpy(pairs, pr.data(), sizeof(str_er_line_pair) * pr.size());
    if (bits && out_words) {
        // the footprints back as they lie on the device (64-bit words over the union of the pre-image boxes), cut to the foot boxes
        std::vector<uint64_t> dev((size_t)T.words);
        HIP_TRY(c, hipMemcpy(dev.data(), c->d_foot_bits, 8 * (size_t)T.words, hipMemcpyDeviceToHost));
        uint32_t *out = bits;
        for (int32_t t = 0; t < n_lines; ++t) {
            const str_er_line_foot &F = ft[(size_t)t];
            const FootLine &L = T.lines[(size_t)t];
            const uint32_t pitch32 = ((uint32_t)F.w + 31u) / 32u;
            for (int32_t rr = 0; rr < F.h; ++rr) {
                const uint64_t *row = dev.data() + L.word_off + (uint64_t)(F.y - L.y + rr) * L.pitch;
                for (uint32_t k = 0; k < pitch32; ++k) {
                    const uint32_t off = (uint32_t)(F.x - L.x) + 32u * k, q = off >> 6, sh = off & 63u;
                    uint64_t v = q < L.pitch ? row[q] >> sh : 0ull;
                    if (sh && q + 1 < L.pitch) v |= row[q + 1] << (64u - sh);
                    *out++ = (uint32_t)v;
                }
            }
        }
    }
    return STR_ER_OK;
} ABI_GUARD(c)

const str_er_line_foot *str_er_result_line_feet(const str_er_result *r, int32_t *n) { return result_table(r, r && r->have_frame_lines, &str_er_result::line_feet, n); }

const str_er_line_pair *str_er_result_line_pairs(const str_er_result *r, int32_t *n) { return result_table(r, r && r->have_frame_lines, &str_er_result::line_pairs, n); }

const str_er_frame_line *str_er_result_frame_lines(const str_er_result *r, int32_t *n) { return result_table(r, r && r->have_frame_lines, &str_er_result::frame_lines, n); }

const int32_t *str_er_result_frame_line_members(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_frame_lines, &str_er_result::frame_line_members, n);
}

} // extern "C"
