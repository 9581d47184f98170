// example_image_stream.cpp -- the reference's image mode over a folder of photographs (src/main.cpp: one cv::imread + text_detect per
// file) written against the ingest stream of include/str_er.h: photographs of assorted sizes are decoded straight into the page-locked
// staging buffer of a depth-3 stream, submitted as lists (str_er_stream_submit_list), and their results come back in order while the
// next lists upload.  Every photograph is then checked against ERFilter::text_detect_batch on the same lists.
//
//   g++ -std=c++17 -O2 example_image_stream.cpp -I../../include -L../lib -lstr_er_hip -o example_image_stream
//   ./example_image_stream strong.classifier weak.classifier [n_photos [photos_per_list]]
//
// The "folder" is synthetic and seeded (dark strokes on a shaded background, sizes drawn from a fixed set), so the program needs no
// image files.  Prints one line per photograph, then whether the stream agrees with the batch calls; exits non-zero if it does not.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "er_filter_hip.hpp"

using namespace str_er_host;

static const int SIZES[][2] = {{640, 480}, {321, 243}, {517, 333}, {211, 97}, {480, 640}};

struct Photo { uint32_t seed; int w, h; };

// The "decoder": photo p as interleaved 8-bit BGR rows of `stride` bytes at dst.
static void decode(const Photo &p, uint8_t *dst, int64_t stride)
{
    uint32_t s = p.seed * 2654435761u + 12345u;
    auto rnd = [&s]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    const int bg[3] = {(int)(150 + rnd() % 90), (int)(150 + rnd() % 90), (int)(150 + rnd() % 90)};
    for (int y = 0; y < p.h; ++y)
        for (int x = 0; x < p.w; ++x)
            for (int c = 0; c < 3; ++c) dst[(size_t)y * stride + 3 * (size_t)x + c] = (uint8_t)std::min(255, bg[c] + (x + 2 * y) % 23);
    const int strokes = 20 + (int)(rnd() % 40);
    for (int k = 0; k < strokes; ++k) {        // letter-sized strokes in a dark colour
        const int sw = 3 + (int)(rnd() % 6), sh = 10 + (int)(rnd() % 30);
        const bool tall = rnd() & 1;
        const int bw = tall ? sw : sh, bh = tall ? sh : sw;
        if (bw >= p.w || bh >= p.h) continue;
        const int x0 = (int)(rnd() % (uint32_t)(p.w - bw)), y0 = (int)(rnd() % (uint32_t)(p.h - bh));
        const int ink[3] = {(int)(rnd() % 60), (int)(rnd() % 60), (int)(rnd() % 60)};
        for (int y = y0; y < y0 + bh; ++y)
            for (int x = x0; x < x0 + bw; ++x)
                for (int c = 0; c < 3; ++c) dst[(size_t)y * stride + 3 * (size_t)x + c] = (uint8_t)ink[c];
    }
}

static bool same_ers(const ERs &a, const ERs &b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i]->key != b[i]->key || a[i]->area != b[i]->area || a[i]->level != b[i]->level || a[i]->score_strong != b[i]->score_strong ||
            a[i]->score_weak != b[i]->score_weak)
            return false;
    return true;
}

struct Unpacked {
    std::vector<std::vector<ERTree>> trees;
    std::vector<ERs> root;
    std::vector<std::vector<ERs>> pool, strong, weak;
};

static bool same_frame(const Unpacked &a, const Unpacked &b, size_t f)
{
    if (a.trees[f].size() != b.trees[f].size()) return false;
    for (size_t i = 0; i < a.trees[f].size(); ++i) {
        const std::vector<ER> &x = a.trees[f][i].nodes, &y = b.trees[f][i].nodes;
        if (x.size() != y.size() || !same_ers(a.pool[f][i], b.pool[f][i]) || !same_ers(a.strong[f][i], b.strong[f][i]) ||
            !same_ers(a.weak[f][i], b.weak[f][i]))
            return false;
        for (size_t k = 0; k < x.size(); ++k)
            if (x[k].key != y[k].key || x[k].area != y[k].area || x[k].level != y[k].level) return false;
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s strong.classifier weak.classifier [n_photos [photos_per_list]]\n", argv[0]); return 2; }
    const int n = argc > 3 ? std::atoi(argv[3]) : 14, per_list = argc > 4 ? std::atoi(argv[4]) : 4;
    if (n < 1 || per_list < 1) { std::fprintf(stderr, "n_photos and photos_per_list are positive\n"); return 2; }
    std::vector<Photo> photos((size_t)n);
    int max_w = 1, max_h = 1;
    for (int i = 0; i < n; ++i) {
        const int *sz = SIZES[(i * 7 + 3) % (int)(sizeof(SIZES) / sizeof(SIZES[0]))];
        photos[(size_t)i] = Photo{(uint32_t)(1000 + i), sz[0], sz[1]};
        max_w = std::max(max_w, sz[0]); max_h = std::max(max_h, sz[1]);
    }
    const uint32_t stages = STR_ER_STAGE_ALL | STR_ER_WANT_NODES;
    str_er_params p;
    str_er_default_params(&p);
    p.thresh_step = 8; p.min_area = 120; p.max_area = 900000; p.stability_t = 2; p.overlap_coef = 0.7;      // (as er_filter below)
    p.max_width = max_w; p.max_height = max_h; p.max_frames = per_list;

    // ---- the stream: 3 lists in flight; each photograph decoded straight into the staging buffer
    str_er_stream *st = nullptr;
    if (str_er_stream_create(&p, 3, &st) != STR_ER_OK) { std::fprintf(stderr, "str_er_stream_create: %s\n", str_er_last_error(nullptr)); return 3; }
    if (str_er_stream_load_cascade(st, STR_ER_CASCADE_STRONG, argv[1]) != STR_ER_OK ||
        str_er_stream_load_cascade(st, STR_ER_CASCADE_WEAK, argv[2]) != STR_ER_OK) {
        std::fprintf(stderr, "load_cascade: %s\n", str_er_stream_last_error(st));
        str_er_stream_destroy(st);
        return 3;
    }
    std::vector<Unpacked> got;                 // per list, in ticket order
    bool ok = true;
    auto collect = [&]() {
        str_er_result *r = nullptr;
        uint64_t ticket = 0;
        if (str_er_stream_next(st, &r, &ticket) != STR_ER_OK) { std::fprintf(stderr, "next: %s\n", str_er_stream_last_error(st)); ok = false; return; }
        if (ticket != got.size() + 1) { std::fprintf(stderr, "ticket %llu out of order\n", (unsigned long long)ticket); ok = false; }
        const int f0 = (int)got.size() * per_list;
        got.emplace_back();
        Unpacked &u = got.back();
        try {
            ERFilter::unpack_batch(r, (size_t)std::min(per_list, n - f0), u.trees, u.root, u.pool, u.strong, u.weak);
        } catch (const std::exception &e) { std::fprintf(stderr, "unpack: %s\n", e.what()); ok = false; }
        str_er_result_free(r);
    };
    for (int f0 = 0; f0 < n && ok; f0 += per_list) {
        if (str_er_stream_pending(st) == str_er_stream_depth(st)) collect();
        int32_t slot; uint8_t *buf; int64_t cap;
        if (str_er_stream_acquire(st, &slot, &buf, &cap) != STR_ER_OK) { std::fprintf(stderr, "acquire: %s\n", str_er_stream_last_error(st)); ok = false; break; }
        const int k = std::min(per_list, n - f0);
        std::vector<str_er_image_ref> refs((size_t)k);
        int64_t at = 0;
        for (int i = 0; i < k; ++i) {          // wherever the decoder likes: here back to back, rows of the photograph's own width
            const Photo &ph = photos[(size_t)(f0 + i)];
            const int64_t stride = 3 * (int64_t)ph.w;
            if (at + stride * ph.h > cap) { std::fprintf(stderr, "staging buffer too small\n"); ok = false; break; }
            decode(ph, buf + at, stride);
            refs[(size_t)i].data = buf + at; refs[(size_t)i].w = ph.w; refs[(size_t)i].h = ph.h; refs[(size_t)i].stride = stride;
            at += stride * ph.h;
        }
        if (!ok) break;
        if (str_er_stream_submit_list(st, slot, refs.data(), k, stages, nullptr) != STR_ER_OK) {
            std::fprintf(stderr, "submit_list: %s\n", str_er_stream_last_error(st));
            ok = false;
        }
    }
    while (ok && str_er_stream_pending(st)) collect();
    str_er_stream_destroy(st);
    if (!ok) return 3;

    // ---- the same lists through ERFilter::text_detect_batch
    try {
        ERFilter er_filter(8, 120, 900000, 2, 0.7, 0.15, max_w, max_h, per_list);
        er_filter.set_stc(argv[1]);
        er_filter.set_wtc(argv[2]);
        bool same = got.size() == (size_t)((n + per_list - 1) / per_list);
        for (int f0 = 0, li = 0; same && f0 < n; f0 += per_list, ++li) {
            const int k = std::min(per_list, n - f0);
            std::vector<std::vector<uint8_t>> pix((size_t)k);
            std::vector<Image8> frames;
            for (int i = 0; i < k; ++i) {
                const Photo &ph = photos[(size_t)(f0 + i)];
                pix[(size_t)i].resize((size_t)ph.w * ph.h * 3);
                decode(ph, pix[(size_t)i].data(), 3 * (int64_t)ph.w);
                frames.emplace_back(pix[(size_t)i].data(), ph.w, ph.h, 3 * (int64_t)ph.w, 3);
            }
            Unpacked want;
            er_filter.text_detect_batch(frames, want.trees, want.root, want.pool, want.strong, want.weak);
            for (int i = 0; i < k; ++i) {
                const Unpacked &g = got[(size_t)li];
                size_t pool = 0, strong = 0, weak = 0;
                for (size_t j = 0; j < g.trees[(size_t)i].size(); ++j)
                    pool += g.pool[(size_t)i][j].size(), strong += g.strong[(size_t)i][j].size(), weak += g.weak[(size_t)i][j].size();
                std::printf("photo %d %dx%d planes %zu pool %zu strong %zu weak %zu\n", f0 + i, photos[(size_t)(f0 + i)].w, photos[(size_t)(f0 + i)].h,
                            g.trees[(size_t)i].size(), pool, strong, weak);
                same = same && same_frame(g, want, (size_t)i);
            }
        }
        std::printf("stream == batch: %s\n", same ? "yes" : "NO");
        return same ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
}
