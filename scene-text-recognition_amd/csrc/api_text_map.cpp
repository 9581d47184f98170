// api_text_map.cpp -- the C ABI, part 7: the frame-resolution text map and line-id map of every frame (STR_ER_WANT_TEXT_MAP /
// _LINE_MAP in run_batch, str_er_text_map_regions on one host plane) and the result accessors of the maps.
// The host lists the contributing regions, computes their pre-image boxes in frame pixels (the exact inverse of the pixel rule of
// str_er_frame_map), bins them into tiles of the frames' maps and lays out the xs / ys tables; k_text_map (er_text_map.inl) gathers.
#include "str_er_ctx.h"

namespace str_er_host {

// the first frame coordinate x in [0, W] whose sample ((2x + 1) * wp) / (2W) is >= a
int32_t first_sample_at(int64_t a, int64_t W, int64_t wp)
{
    const int64_t num = 2 * W * a - wp, den = 2 * wp;
    const int64_t x = num <= 0 ? 0 : (num + den - 1) / den;
    return (int32_t)std::min<int64_t>(x, W);
}

uint32_t SampleTabs::table(int32_t n, int32_t np)
{
    const auto it = at.find({n, np});
    if (it != at.end()) return it->second;
    const uint32_t first = (uint32_t)tabs.size();
    for (int64_t x = 0; x < n; ++x) tabs.push_back((uint16_t)(((2 * x + 1) * (int64_t)np) / (2 * (int64_t)n)));
    at.emplace(std::make_pair(n, np), first);
    return first;
}

namespace {

// where the ids sit behind the bytes in c->tmap, and the bytes the maps of n_elem elements need
void tmap_out_offsets(uint64_t n_elem, bool map, bool ids, size_t &o_ids, size_t &need)
{
    o_ids = map ? align_up((size_t)n_elem, 256) : 0;
    need = o_ids + (ids ? 4 * (size_t)n_elem : 0);
}

// One region of the stage, before binning: its frame, the level size of its plane, its box and mask, what it contributes
struct TmapRegion {
    uint32_t frame;
    int32_t  pw, ph;
    uint16_t x, y, w, h;
    uint64_t word_off;
    uint32_t value;
    int32_t  id;
};

// The tables of one launch: tiles | list | regions | xs / ys tables
struct TmapLayout {
    std::vector<TextMapTile> tiles;
    std::vector<uint32_t>    list;
    std::vector<TextMapCand> cands;
    std::vector<uint16_t>    tabs;
};

// frames[f] = (W, H, off); the regions binned into the frames' tiles (a tile: TMAP_CHUNK_ELEMS * ceil(W / TMAP_CHUNK_ELEMS) elements,
// at least a row, so a region's tiles are those from its first pre-image element's to its last's: a gap between two of its rows is
// shorter than a row and holds no whole tile)
void tmap_layout(const std::vector<str_er_frame_map> &frames, const std::vector<TmapRegion> &regs, TmapLayout &L)
{
    std::vector<uint32_t> tile_base(frames.size() + 1, 0), tile_len(frames.size());
    for (size_t f = 0; f < frames.size(); ++f) {
        const uint64_t W = (uint64_t)frames[f].width, span = ((uint64_t)frames[f].width * (uint64_t)frames[f].height + 3u) & ~(uint64_t)3u;
        tile_len[f] = (uint32_t)(TMAP_CHUNK_ELEMS * ((W + TMAP_CHUNK_ELEMS - 1) / TMAP_CHUNK_ELEMS));
        tile_base[f + 1] = tile_base[f] + (uint32_t)((span + tile_len[f] - 1) / tile_len[f]);
    }
    L.tiles.assign(tile_base.back(), TextMapTile{});
    for (size_t f = 0; f < frames.size(); ++f) {
        const uint64_t span = ((uint64_t)frames[f].width * (uint64_t)frames[f].height + 3u) & ~(uint64_t)3u;
        for (uint32_t t = tile_base[f]; t < tile_base[f + 1]; ++t) {
            TextMapTile &T = L.tiles[t];
            T.off = frames[f].off; T.e0 = (t - tile_base[f]) * tile_len[f];
            T.n_elem = (uint32_t)std::min<uint64_t>(tile_len[f], span - T.e0);
            T.width = frames[f].width; T.height = frames[f].height;
        }
    }
    // the xs / ys tables, one per (frame size, level size) pair
    SampleTabs st;
    auto table = [&](int32_t n, int32_t np) -> uint32_t { return st.table(n, np); };
    L.cands.clear();
    std::vector<std::pair<uint32_t, uint32_t>> range;         // (first tile, last tile) of every region kept
    for (const TmapRegion &g : regs) {
        const str_er_frame_map &F = frames[g.frame];
        TextMapCand C{};
        C.word_off = g.word_off; C.pitch = (g.w + 31u) / 32u; C.x = g.x; C.y = g.y; C.w = g.w; C.h = g.h;
        C.fx0 = first_sample_at(g.x, F.width, g.pw); C.fx1 = first_sample_at((int64_t)g.x + g.w, F.width, g.pw);
        C.fy0 = first_sample_at(g.y, F.height, g.ph); C.fy1 = first_sample_at((int64_t)g.y + g.h, F.height, g.ph);
        if (C.fx0 >= C.fx1 || C.fy0 >= C.fy1) continue;         // (upsampled: no frame pixel samples the box)
        C.xtab = table(F.width, g.pw); C.ytab = table(F.height, g.ph);
        C.value = g.value; C.id = g.id;
        const uint64_t W = (uint64_t)F.width;
        const uint64_t first = (uint64_t)C.fy0 * W + (uint64_t)C.fx0, last = (uint64_t)(C.fy1 - 1) * W + (uint64_t)(C.fx1 - 1);
        range.emplace_back(tile_base[g.frame] + (uint32_t)(first / tile_len[g.frame]), tile_base[g.frame] + (uint32_t)(last / tile_len[g.frame]));
        L.cands.push_back(C);
    }
    // the CSR tile -> regions (a counting sort, regions in order)
    for (const auto &rg : range)
        for (uint32_t t = rg.first; t <= rg.second; ++t) ++L.tiles[t].count;
    uint32_t at = 0;
    for (TextMapTile &T : L.tiles) { T.first = at; at += T.count; T.count = 0; }
    L.list.assign(at, 0);
    for (uint32_t k = 0; k < (uint32_t)range.size(); ++k)
        for (uint32_t t = range[k].first; t <= range[k].second; ++t) { TextMapTile &T = L.tiles[t]; L.list[T.first + T.count++] = k; }
    L.tabs.swap(st.tabs);
    if (L.tabs.empty()) L.tabs.push_back(0);
}

// the launch of one layout on s (the maps into c->tmap, sized by text_map_reserve / the caller), one copy back, one wait;
// n_elem elements of map bytes and / or ids to out_map / out_ids
int tmap_stage(str_er_ctx *c, hipStream_t s, const TmapLayout &L, const uint32_t *d_bits, uint64_t n_elem, uint8_t *out_map, int32_t *out_ids,
               bool in_batch)
{
    const bool map = out_map != nullptr, ids = out_ids != nullptr;
    size_t o_ids, need;
    tmap_out_offsets(n_elem, map, ids, o_ids, need);
    if (need > c->tmap.size()) return fail(c, STR_ER_EHIP, "text map: the output buffer was not sized (internal error)");
    const size_t o_list = align_up(sizeof(TextMapTile) * L.tiles.size(), 256), o_cand = align_up(o_list + 4 * L.list.size(), 256);
    const size_t o_tab = align_up(o_cand + sizeof(TextMapCand) * L.cands.size(), 256), tab_need = o_tab + 2 * L.tabs.size();
    const int rc = c->tmap_tab.ensure(c, tab_need, "text map tables");
    if (rc != STR_ER_OK) return rc;
    std::memcpy(c->tmap_tab.h(), L.tiles.data(), sizeof(TextMapTile) * L.tiles.size());
    if (!L.list.empty()) std::memcpy(c->tmap_tab.h() + o_list, L.list.data(), 4 * L.list.size());
    if (!L.cands.empty()) std::memcpy(c->tmap_tab.h() + o_cand, L.cands.data(), sizeof(TextMapCand) * L.cands.size());
    std::memcpy(c->tmap_tab.h() + o_tab, L.tabs.data(), 2 * L.tabs.size());
    HIP_TRY(c, hipMemcpyAsync(c->tmap_tab.d(), c->tmap_tab.h(), tab_need, hipMemcpyHostToDevice, s));
    launch_text_map(s, reinterpret_cast<const TextMapTile *>(c->tmap_tab.d()), (int)L.tiles.size(), reinterpret_cast<const uint32_t *>(c->tmap_tab.d() + o_list),
                    reinterpret_cast<const TextMapCand *>(c->tmap_tab.d() + o_cand), reinterpret_cast<const uint16_t *>(c->tmap_tab.d() + o_tab), d_bits,
                    map ? c->tmap.d() : nullptr, ids ? reinterpret_cast<int32_t *>(c->tmap.d() + o_ids) : nullptr);
    HIP_TRY(c, hipGetLastError());
    if (in_batch) rec(c, "text_map");          // (the call's one profiling event of the stage)
    HIP_TRY(c, hipMemcpyAsync(c->tmap.h(), c->tmap.d(), need, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    if (map) std::memcpy(out_map, c->tmap.h(), (size_t)n_elem);
    if (ids) std::memcpy(out_ids, c->tmap.h() + o_ids, 4 * (size_t)n_elem);
    return STR_ER_OK;
}

uint64_t frame_span(int32_t w, int32_t h) { return ((uint64_t)w * (uint64_t)h + 3u) & ~(uint64_t)3u; }

} // namespace

// the output maps of n_elem elements in c->tmap
static int reserve_out(str_er_ctx *c, uint64_t n_elem, bool map, bool ids)
{
    size_t o_ids, need;
    tmap_out_offsets(n_elem, map, ids, o_ids, need);
    return c->tmap.ensure(c, need, "text maps");
}

int text_map_reserve(str_er_ctx *c, uint32_t stages, const std::vector<int32_t> &frame_wh)
{
    const bool map = (stages & STR_ER_WANT_TEXT_MAP) != 0, ids = (stages & STR_ER_WANT_LINE_MAP) != 0;
    if (!map && !ids) return STR_ER_OK;
    uint64_t n_elem = 0;
    for (size_t f = 0; f + 1 < frame_wh.size(); f += 2) {
        if (frame_wh[f] > 65535 || frame_wh[f + 1] > 65535) return fail(c, STR_ER_ECAPACITY, "text map: a frame wider or taller than 65535 pixels");
        n_elem += frame_span(frame_wh[f], frame_wh[f + 1]);
    }
    return reserve_out(c, n_elem, map, ids);
}

int text_map_phase(str_er_ctx *c, hipStream_t s, const Batch &b, uint32_t stages, float qscale, const uint32_t *d_mask_bits, str_er_result *r,
                   const uint32_t **d_made_bits, std::vector<uint64_t> *made_word_off)
{
    const bool map = (stages & STR_ER_WANT_TEXT_MAP) != 0, ids = (stages & STR_ER_WANT_LINE_MAP) != 0;
    const size_t n_frames = b.frame_wh.size() / 2, total = r->cands.size();
    r->frame_maps.resize(n_frames);
    uint64_t n_elem = 0;
    for (size_t f = 0; f < n_frames; ++f) {
        str_er_frame_map &F = r->frame_maps[f];
        F.off = n_elem; F.width = b.frame_wh[2 * f]; F.height = b.frame_wh[2 * f + 1];
        n_elem += frame_span(F.width, F.height);
    }
    // what every candidate contributes: its class bits, and as a member of lines bit 4, bit 8 (kept in an alive line) and the smallest line
    std::vector<uint32_t> value(total, 0);
    std::vector<int32_t>  line(total, INT32_MAX);
    for (size_t k = 0; k < total; ++k) value[k] = r->cands[k].cls == STR_ER_CLS_STRONG ? STR_ER_TEXT_MAP_STRONG : r->cands[k].cls == STR_ER_CLS_WEAK ? STR_ER_TEXT_MAP_WEAK : 0u;
    if (r->have_texts)
        for (size_t t = 0; t < r->texts.size(); ++t) {
            const str_er_text &tx = r->texts[t];
            const bool alive = r->have_line_ocr && r->text_alive[t] != 0;
            for (int32_t m = 0; m < tx.count; ++m) {
                const size_t e = (size_t)tx.first + (size_t)m, k = (size_t)r->text_ers[e];
                value[k] |= STR_ER_TEXT_MAP_LINE | (alive && r->line_kept[e] ? STR_ER_TEXT_MAP_OCR : 0u);
                line[k] = std::min(line[k], (int32_t)t);
            }
        }
    std::vector<uint32_t> who;            // the contributing candidates, in order
    for (uint32_t k = 0; k < (uint32_t)total; ++k) {
        if (r->cands[k].cls == STR_ER_CLS_POOL) continue;
        if (!(map || line[k] != INT32_MAX)) continue;
        if (r->cands[k].w > MASK_MAX_WIDTH)
            return fail(c, STR_ER_ECAPACITY, "STR_ER_WANT_TEXT_MAP / _LINE_MAP: a candidate wider than " + std::to_string(MASK_MAX_WIDTH) + " pixels");
        who.push_back(k);
    }
    std::vector<TmapRegion> regs(who.size());
    const uint32_t *d_bits = d_mask_bits;
    if (d_mask_bits) {
        // the masks of this call (STR_ER_WANT_MASKS / _SHAPES / _STROKES) are still on the device: the same words, indexed as in the result
        for (size_t i = 0; i < who.size(); ++i) regs[i].word_off = r->masks[who[i]].word_off;
    } else if (!who.empty()) {
        // the masks of the contributing candidates, made by the mask kernels and left on the device
        std::vector<MaskJob> mj(who.size());
        uint64_t words = 0;
        for (size_t i = 0; i < who.size(); ++i) {
            const str_er_cand &cd = r->cands[who[i]];
            const PlaneDesc   &pd = b.planes[cd.plane];
            MaskJob &m = mj[i];
            m.pix = pd.pix; m.stride = pd.stride; m.invert = (uint32_t)pd.invert; m.plane_w = (uint32_t)pd.w; m.key = cd.key;
            m.x = cd.x; m.y = cd.y; m.w = cd.w; m.h = cd.h; m.level = cd.level; m.idx = (uint32_t)i; m.out_off = words; m.scratch_off = 0;
            regs[i].word_off = words;
            words += (uint64_t)cd.h * ((cd.w + 31u) / 32u);
        }
        const int rcm = mask_launch(c, s, mj, words, qscale, &d_bits);
        if (rcm != STR_ER_OK) return rcm;
        if (d_made_bits && made_word_off) {        // (STR_ER_WANT_FRAME_LINES behind the maps: the same words serve it)
            *d_made_bits = d_bits;
            made_word_off->assign(total, UINT64_MAX);
            for (size_t i = 0; i < who.size(); ++i) (*made_word_off)[who[i]] = regs[i].word_off;
        }
    }
    for (size_t i = 0; i < who.size(); ++i) {
        const str_er_cand &cd = r->cands[who[i]];
        const PlaneDesc   &pd = b.planes[cd.plane];
        TmapRegion &g = regs[i];
        g.frame = cd.frame; g.pw = pd.w; g.ph = pd.h; g.x = cd.x; g.y = cd.y; g.w = cd.w; g.h = cd.h;
        g.value = value[who[i]]; g.id = line[who[i]];
        if (g.frame >= n_frames) return fail(c, STR_ER_EHIP, "text map: a candidate of no frame (internal error)");
    }
    const auto t0 = std::chrono::steady_clock::now();
    TmapLayout L;
    tmap_layout(r->frame_maps, regs, L);
    if (c->dbg_stats)        // developer aid (tools/dev_text_map.py --bin-stats): the host side of the stage
        std::fprintf(stderr, "[str_er] text map: %zu regions, %zu tiles, %zu list entries, %zu table entries, binning %.3f ms, %llu elements back\n",
                     L.cands.size(), L.tiles.size(), L.list.size(), L.tabs.size(),
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
                     (unsigned long long)n_elem * ((map ? 1u : 0u) + (ids ? 4u : 0u)));
    if (map) r->text_map.resize((size_t)n_elem);
    if (ids) r->line_map.resize((size_t)n_elem);
    const int rc = tmap_stage(c, s, L, d_bits, n_elem, map ? r->text_map.data() : nullptr, ids ? r->line_map.data() : nullptr, true);
    if (rc != STR_ER_OK) return rc;
    r->have_text_map = map;
    r->have_line_map = ids;
    return STR_ER_OK;
}

} // namespace str_er_host

extern "C" {

int str_er_text_map_regions(str_er_ctx *c, const uint8_t *plane, int32_t w, int32_t h, int64_t stride, const str_er_cand *regions,
                            const uint8_t *values, const int32_t *ids, int32_t n, int32_t out_w, int32_t out_h, uint8_t *out_map, int32_t *out_ids)
try {
    if (!c) return STR_ER_EINVAL;
    if (out_w < 1 || out_h < 1 || !out_map || (ids == nullptr) != (out_ids == nullptr) || (n > 0 && !values))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    if (out_w > 65535 || out_h > 65535) return fail(c, STR_ER_ECAPACITY, "text map: an output wider or taller than 65535 pixels");
    const DetectParams dp = make_dp(c);
    std::vector<MaskJob> jobs;
    uint64_t words = 0;
    int rc = region_jobs(c, plane, w, h, stride, regions, n, dp, jobs, words);
    if (rc != STR_ER_OK) return rc;
    for (int32_t i = 0; ids && i < n; ++i)
        if (ids[i] < 0 || ids[i] == INT32_MAX) return fail(c, STR_ER_EINVAL, "region " + std::to_string(i) + ": id outside [0, 2^31 - 2]");
    HIP_TRY(c, hipSetDevice(c->prm.device));
    if ((rc = reserve_out(c, frame_span(out_w, out_h), true, ids != nullptr)) != STR_ER_OK) return rc;
    std::vector<str_er_frame_map> frames(1);
    frames[0].off = 0; frames[0].width = out_w; frames[0].height = out_h;
    std::vector<TmapRegion> regs((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        const str_er_cand &g = regions[i];
        TmapRegion &q = regs[(size_t)i];
        q.frame = 0; q.pw = w; q.ph = h; q.x = g.x; q.y = g.y; q.w = g.w; q.h = g.h; q.word_off = jobs[(size_t)i].out_off;
        q.value = values[i]; q.id = ids ? ids[i] : INT32_MAX;
    }
    const uint32_t *d_bits = nullptr;
    if (n > 0) {
        if ((rc = region_upload(c, plane, w, h, stride, jobs)) != STR_ER_OK) return rc;
        if ((rc = mask_launch(c, c->stream, jobs, words, dp.qscale, &d_bits)) != STR_ER_OK) return rc;
    }
    TmapLayout L;
    tmap_layout(frames, regs, L);
    const uint64_t n_elem = frame_span(out_w, out_h), px = (uint64_t)out_w * (uint64_t)out_h;
    std::vector<uint8_t> m((size_t)n_elem);
    std::vector<int32_t> d(ids ? (size_t)n_elem : 0);
    if ((rc = tmap_stage(c, c->stream, L, d_bits, n_elem, m.data(), ids ? d.data() : nullptr, false)) != STR_ER_OK) return rc;
    std::memcpy(out_map, m.data(), (size_t)px);
    if (ids) std::memcpy(out_ids, d.data(), 4 * (size_t)px);
    return STR_ER_OK;
} ABI_GUARD(c)

const str_er_frame_map *str_er_result_frame_maps(const str_er_result *r, int32_t *n) { return result_table(r, r && (r->have_text_map || r->have_line_map), &str_er_result::frame_maps, n); }

const uint8_t *str_er_result_text_map_pixels(const str_er_result *r, uint64_t *n_bytes) { return result_table(r, r && r->have_text_map, &str_er_result::text_map, n_bytes); }

const int32_t *str_er_result_line_map_ids(const str_er_result *r, uint64_t *n)
{
    static const int32_t no_line = -1;        // (an empty map: a pointer to -1)
    return result_table(r, r && r->have_line_map, &str_er_result::line_map, n, no_line);
}

} // extern "C"
