// api_line_crops.cpp -- the C ABI, part 6: the rectified image of every text line (STR_ER_WANT_LINE_CROPS / _GLYPHS in run_batch,
// str_er_line_crops on one host plane, str_er_line_crop_geometry, str_er_set_line_crop) and the result accessors of the crops.
// The geometry is host f64 in the order str_er.h states (the build has -ffp-contract=off); the pixels come from k_line_crops.
#include "str_er_ctx.h"

#include <map>

namespace str_er_host {

namespace {

bool crop_settings_ok(int32_t height, int32_t max_width, double pad)
{
    return height >= 8 && height <= 256 && max_width >= 1 && max_width <= 8192 && pad >= 0.0 && pad <= 1.0;
}

bool to_fixed(double v, int32_t &out)
{
    const double f = 65536.0 * v;
    if (!(f > -2147483648.0 && f < 2147483647.0)) return false;         // (also false for NaN)
    out = (int32_t)std::llround(f);
    return true;
}

// the crop layout: crop k from a multiple of 4 bytes on, width * height bytes
uint64_t crop_span(const str_er_line_crop &g)
{
    return ((uint64_t)g.width * (uint64_t)g.height + 3u) & ~(uint64_t)3u;
}

// the crops of `jobs` (out_off set, n_bytes in all): uploaded, launched on s, one copy back through the page-locked buffer, one wait.
// Glyph crops when d_bits is set (members index the words there).
int crop_stage(str_er_ctx *c, hipStream_t s, const std::vector<LineCropJob> &jobs, const std::vector<GlyphMember> &members, const uint32_t *d_bits,
               uint64_t n_bytes, uint8_t *grey, uint8_t *glyph, bool in_batch)
{
    const size_t n = jobs.size();
    if (n == 0) return STR_ER_OK;
    const size_t o_mem = align_up(sizeof(LineCropJob) * n, 256), o_pix = align_up(o_mem + sizeof(GlyphMember) * members.size(), 256);
    const size_t o_glyph = o_pix + (size_t)n_bytes, need = o_glyph + (d_bits ? (size_t)n_bytes : 0);
    const int rc = c->crop.ensure(c, need, "line crops");         // (jobs | members | grey | glyph)
    if (rc != STR_ER_OK) return rc;
    std::memcpy(c->crop.h(), jobs.data(), sizeof(LineCropJob) * n);
    if (!members.empty()) std::memcpy(c->crop.h() + o_mem, members.data(), sizeof(GlyphMember) * members.size());
    HIP_TRY(c, hipMemcpyAsync(c->crop.d(), c->crop.h(), o_pix, hipMemcpyHostToDevice, s));
    launch_line_crops(s, reinterpret_cast<const LineCropJob *>(c->crop.d()), (int)n, c->crop.d() + o_pix, d_bits ? c->crop.d() + o_glyph : nullptr,
                      reinterpret_cast<const GlyphMember *>(c->crop.d() + o_mem), d_bits);
    HIP_TRY(c, hipGetLastError());
    if (in_batch) rec(c, "line_crops");         // (the call's one profiling event of the stage)
    HIP_TRY(c, hipMemcpyAsync(c->crop.h() + o_pix, c->crop.d() + o_pix, need - o_pix, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    std::memcpy(grey, c->crop.h() + o_pix, (size_t)n_bytes);
    if (d_bits) std::memcpy(glyph, c->crop.h() + o_glyph, (size_t)n_bytes);
    return STR_ER_OK;
}

void fill_job(LineCropJob &j, const str_er_line_crop &g, const uint8_t *pix, int32_t stride, int32_t pw, int32_t ph)
{
    j.pix = pix; j.out_off = g.pix_off; j.stride = stride; j.pw = pw; j.ph = ph; j.width = g.width; j.height = g.height;
    j.ax = g.ax; j.ay = g.ay; j.ux = g.ux; j.uy = g.uy; j.vx = g.vx; j.vy = g.vy; j.m_first = 0; j.m_count = 0; j.pad0 = 0;
}

} // namespace

int line_crop_geometry(const int32_t *boxes, int32_t n_boxes, double slope, int32_t height, int32_t max_width, double pad, str_er_line_crop &out)
{
    if (!boxes || n_boxes < 1 || !crop_settings_ok(height, max_width, pad)) return STR_ER_EINVAL;
    const double s = std::isfinite(slope) ? slope : 0.0;        // (fitline_avgslope divides by zero on a vertical fit)
    const double r = std::sqrt(1.0 + s * s);
    const double dx = 1.0 / r, dy = s / r, nx = -s / r, ny = 1.0 / r;
    double u0 = 0, u1 = 0, v0 = 0, v1 = 0;
    for (int32_t k = 0; k < n_boxes; ++k) {
        const int32_t *b = boxes + 4 * (size_t)k;
        if (b[2] < 1 || b[3] < 1) return STR_ER_EINVAL;
        for (int q = 0; q < 4; ++q) {
            const double cx = (double)((int64_t)b[0] + ((q & 1) ? b[2] : 0)), cy = (double)((int64_t)b[1] + ((q & 2) ? b[3] : 0));
            const double u = cx * dx + cy * dy, v = cx * nx + cy * ny;
            if (k == 0 && q == 0) { u0 = u1 = u; v0 = v1 = v; continue; }
            u0 = std::min(u0, u); u1 = std::max(u1, u); v0 = std::min(v0, v); v1 = std::max(v1, v);
        }
    }
    const double p = pad * (v1 - v0);
    const double U0 = u0 - p, U1 = u1 + p, V0 = v0 - p, V1 = v1 + p;
    const double kv = (V1 - V0) / height;
    const double wd = std::min((double)max_width, std::max(1.0, std::ceil((U1 - U0) / kv)));
    if (!(wd >= 1.0)) return STR_ER_EINVAL;
    const int32_t width = (int32_t)wd;
    const double  ku = (U1 - U0) / width;
    const double  ax = U0 * dx + V0 * nx + 0.5 * ku * dx + 0.5 * kv * nx - 0.5;
    const double  ay = U0 * dy + V0 * ny + 0.5 * ku * dy + 0.5 * kv * ny - 0.5;
    str_er_line_crop g{};
    g.width = width; g.height = height;
    if (!to_fixed(ax, g.ax) || !to_fixed(ay, g.ay) || !to_fixed(ku * dx, g.ux) || !to_fixed(ku * dy, g.uy) || !to_fixed(kv * nx, g.vx) ||
        !to_fixed(kv * ny, g.vy))
        return STR_ER_EINVAL;
    out = g;
    return STR_ER_OK;
}

int line_crop_phase(str_er_ctx *c, hipStream_t s, const Batch &b, float qscale, bool glyphs, const uint32_t *d_mask_bits, str_er_result *r)
{
    const size_t n = r->texts.size();
    // the Y plane of every image: any of its planes finds it through color_pitch (PlaneDesc)
    std::map<uint64_t, const PlaneDesc *> ys;
    for (const PlaneDesc &pd : b.planes) ys.emplace(((uint64_t)pd.frame << 8) | pd.pyr, &pd);
    std::vector<LineCropJob>      jobs(n);
    std::vector<GlyphMember>      members;
    std::vector<int32_t>          boxes;
    std::vector<uint32_t>         mem_cand;        // glyphs: the candidate of every member record
    r->line_crops.resize(n);
    uint64_t bytes = 0;
    for (size_t t = 0; t < n; ++t) {
        const str_er_text &tx = r->texts[t];
        const auto         it = ys.find(((uint64_t)tx.frame << 8) | tx.pyr);
        if (it == ys.end() || tx.count < 1) return fail(c, STR_ER_EHIP, "line crops: line " + std::to_string(t) + " has no plane (internal error)");
        const PlaneDesc &pd = *it->second;
        boxes.clear();
        for (int32_t k = 0; k < tx.count; ++k) {
            const str_er_gbound &g = r->gbounds[(size_t)r->text_ers[(size_t)tx.first + (size_t)k]];
            boxes.insert(boxes.end(), {g.x, g.y, g.w, g.h});
        }
        str_er_line_crop &g = r->line_crops[t];
        if (line_crop_geometry(boxes.data(), tx.count, tx.slope, c->crop_height, c->crop_max_width, c->crop_pad, g) != STR_ER_OK)
            return fail(c, STR_ER_EINVAL, "line crops: the geometry of line " + std::to_string(t) + " leaves 16.16 fixed point");
        g.pix_off = bytes;
        bytes += crop_span(g);
        LineCropJob &j = jobs[t];
        fill_job(j, g, pd.pix - (size_t)(pd.ch % 3) * pd.color_pitch, pd.stride, pd.w, pd.h);
        if (glyphs) {           // the line's distinct members, in candidate order
            std::vector<uint32_t> m(r->text_ers.begin() + tx.first, r->text_ers.begin() + tx.first + tx.count);
            std::sort(m.begin(), m.end());
            m.erase(std::unique(m.begin(), m.end()), m.end());
            j.m_first = (uint32_t)mem_cand.size(); j.m_count = (uint32_t)m.size();
            mem_cand.insert(mem_cand.end(), m.begin(), m.end());
        }
    }
    r->crop_pixels.assign(bytes, 0);
    const uint32_t *d_bits = nullptr;
    if (glyphs) {
        members.resize(mem_cand.size());
        if (d_mask_bits) {
            // the masks of this call (STR_ER_WANT_MASKS / _SHAPES / _STROKES) are still on the device: the same words, indexed as in the result
            d_bits = d_mask_bits;
            for (size_t k = 0; k < mem_cand.size(); ++k) members[k].word_off = r->masks[mem_cand[k]].word_off;
        } else {
            // the masks of the distinct members of all lines, made by the mask kernels and left on the device
            std::vector<uint32_t> u(mem_cand);
            std::sort(u.begin(), u.end());
            u.erase(std::unique(u.begin(), u.end()), u.end());
            std::vector<MaskJob>  mj(u.size());
            std::vector<uint64_t> off(u.size());
            uint64_t              words = 0;
            for (size_t k = 0; k < u.size(); ++k) {
                const str_er_cand &cd = r->cands[u[k]];
                const PlaneDesc   &pd = b.planes[cd.plane];
                if (cd.w > MASK_MAX_WIDTH) return fail(c, STR_ER_ECAPACITY, "STR_ER_WANT_LINE_GLYPHS: a member wider than " + std::to_string(MASK_MAX_WIDTH) + " pixels");
                MaskJob &m = mj[k];
                m.pix = pd.pix; m.stride = pd.stride; m.invert = (uint32_t)pd.invert; m.plane_w = (uint32_t)pd.w; m.key = cd.key;
                m.x = cd.x; m.y = cd.y; m.w = cd.w; m.h = cd.h; m.level = cd.level; m.idx = (uint32_t)k; m.out_off = words; m.scratch_off = 0;
                off[k] = words;
                words += (uint64_t)cd.h * ((cd.w + 31u) / 32u);
            }
            if (!mj.empty()) {
                const int rcm = mask_launch(c, s, mj, words, qscale, &d_bits);
                if (rcm != STR_ER_OK) return rcm;
            }
            for (size_t k = 0; k < mem_cand.size(); ++k) members[k].word_off = off[(size_t)(std::lower_bound(u.begin(), u.end(), mem_cand[k]) - u.begin())];
        }
        for (size_t k = 0; k < mem_cand.size(); ++k) {
            const str_er_cand &cd = r->cands[mem_cand[k]];
            members[k].x = cd.x; members[k].y = cd.y; members[k].w = cd.w; members[k].h = cd.h;
        }
        r->glyph_pixels.assign(bytes, 0);
        if (!d_bits && n) return fail(c, STR_ER_EHIP, "line glyphs: no mask words (internal error)");
    }
    const int rc = crop_stage(c, s, jobs, members, d_bits, bytes, r->crop_pixels.data(), glyphs ? r->glyph_pixels.data() : nullptr, true);
    if (rc != STR_ER_OK) return rc;
    r->have_line_crops = true;
    r->have_line_glyphs = glyphs;
    return STR_ER_OK;
}

} // namespace str_er_host

extern "C" {

int str_er_set_line_crop(str_er_ctx *c, int32_t height, int32_t max_width, double pad)
try {
    if (!c) return STR_ER_EINVAL;
    if (!crop_settings_ok(height, max_width, pad))
        return fail(c, STR_ER_EINVAL, "line crop: height must be in [8, 256], max_width in [1, 8192], pad in [0, 1]");
    c->crop_height = height; c->crop_max_width = max_width; c->crop_pad = pad;
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_line_crop_geometry(const int32_t *boxes_xywh, int32_t n_boxes, double slope, int32_t height, int32_t max_width, double pad,
                              str_er_line_crop *out)
{
    if (!out) return STR_ER_EINVAL;
    return line_crop_geometry(boxes_xywh, n_boxes, slope, height, max_width, pad, *out);
}

int str_er_line_crops(str_er_ctx *c, const uint8_t *plane, int32_t w, int32_t h, int64_t stride, const int32_t *boxes_xywh,
                      const int32_t *first, const int32_t *count, const double *slopes, int32_t n_lines, uint8_t *pixels, uint64_t cap,
                      uint64_t *n_bytes, str_er_line_crop *recs)
try {
    if (!c) return STR_ER_EINVAL;
    if (!plane || w < 1 || h < 1 || stride < w || n_lines < 0 || !n_bytes || (n_lines > 0 && (!boxes_xywh || !first || !count || !slopes || !recs)))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    uint64_t bytes = 0;
    for (int32_t k = 0; k < n_lines; ++k) {
        const std::string who = "line " + std::to_string(k) + ": ";
        if (first[k] < 0 || count[k] < 1) return fail(c, STR_ER_EINVAL, who + "first < 0 or count < 1");
        if (line_crop_geometry(boxes_xywh + 4 * (size_t)first[k], count[k], slopes[k], c->crop_height, c->crop_max_width, c->crop_pad, recs[k]) != STR_ER_OK)
            return fail(c, STR_ER_EINVAL, who + "a box with w or h < 1, or a geometry outside 16.16 fixed point");
        recs[k].pix_off = bytes;
        bytes += crop_span(recs[k]);
    }
    *n_bytes = bytes;
    if (!pixels || n_lines == 0) return STR_ER_OK;
    if (bytes > cap) return fail(c, STR_ER_ECAPACITY, "the crops need " + std::to_string(bytes) + " bytes, cap is " + std::to_string(cap));
    HIP_TRY(c, hipSetDevice(c->prm.device));
    if ((size_t)w * (size_t)h > c->pix_bytes) return fail(c, STR_ER_ECAPACITY, "plane larger than the context capacity");
    HIP_TRY(c, hipMemcpy2DAsync(c->d_pix, (size_t)w, plane, (size_t)stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice, c->stream));
    std::vector<LineCropJob> jobs((size_t)n_lines);
    for (int32_t k = 0; k < n_lines; ++k) fill_job(jobs[(size_t)k], recs[k], c->d_pix, w, w, h);
    return crop_stage(c, c->stream, jobs, {}, nullptr, bytes, pixels, nullptr, false);
} ABI_GUARD(c)

const str_er_line_crop *str_er_result_line_crops(const str_er_result *r, int32_t *n) { return result_table(r, r && r->have_line_crops, &str_er_result::line_crops, n); }

const uint8_t *str_er_result_line_crop_pixels(const str_er_result *r, uint64_t *n_bytes) { return result_table(r, r && r->have_line_crops, &str_er_result::crop_pixels, n_bytes); }

const uint8_t *str_er_result_line_glyph_pixels(const str_er_result *r, uint64_t *n_bytes) { return result_table(r, r && r->have_line_glyphs, &str_er_result::glyph_pixels, n_bytes); }

} // extern "C"
