// example_er_strokes.cpp -- the stroke-width descriptor of every ER a frame yields (STR_ER_WANT_STROKES), and for plane 0 the same
// descriptors through ERFilter::er_strokes, the single-stage form for ERs of a host plane.
//
//   g++ -std=c++17 -O2 example_er_strokes.cpp -I../../include -L../lib -lstr_er_hip -o example_er_strokes
//   ./example_er_strokes strong.classifier weak.classifier frame.bgr width height
//
// frame.bgr is a raw interleaved 8-bit BGR dump.  Prints "stroke <candidate> <depth_max> <ridge_pixels> <mean ridge depth> <spread>"
// for every candidate of the call, in str_er_result_cands order, then whether the fused and the single-stage records of plane 0 agree
// byte for byte.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

#include "er_filter_hip.hpp"

using namespace str_er_host;

int main(int argc, char **argv)
{
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s strong.classifier weak.classifier frame.bgr width height\n", argv[0]);
        return 2;
    }
    const int w = std::atoi(argv[4]), h = std::atoi(argv[5]);
    if (w < 1 || h < 1) { std::fprintf(stderr, "bad size\n"); return 2; }
    std::vector<uint8_t> pix((size_t)w * h * 3);
    std::ifstream in(argv[3], std::ios::binary);
    if (!in.read(reinterpret_cast<char *>(pix.data()), (std::streamsize)pix.size())) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
    try {
        ERFilter f(8, 120, 900000, 2, 0.7, 0.15, w, h, 1);
        f.set_stc(argv[1]);
        f.set_wtc(argv[2]);
        str_er_result *r = nullptr;
        int rc = str_er_detect_bgr(f.handle(), pix.data(), w, h, 3 * (int64_t)w, 3 * (int64_t)w * h, 1, STR_ER_MEM_HOST,
                                   STR_ER_STAGE_ALL | STR_ER_WANT_STROKES, &r);
        if (rc != STR_ER_OK) { std::fprintf(stderr, "detect: %s\n", str_er_last_error(f.handle())); return 1; }
        std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
        int32_t              n = 0, nk = 0, n0 = 0;
        const str_er_cand   *cands = str_er_result_cands(r, &n);
        const str_er_stroke *strokes = str_er_result_strokes(r, &nk);
        if (!strokes || nk != n) { std::fprintf(stderr, "no strokes\n"); return 1; }
        for (int32_t i = 0; i < n; ++i) {
            const str_er_stroke &s = strokes[i];
            const double m = (double)s.ridge_depth_sum / s.ridge_pixels, spread = (double)s.ridge_depth_sum2 / s.ridge_pixels - m * m;
            std::printf("stroke %d %u %u %.3f %.3f\n", i, s.depth_max, s.ridge_pixels, m, spread);
        }
        // plane 0 (Y) again, through the single-stage call on the plane compute_channels gives
        std::vector<std::vector<uint8_t>> ch;
        f.compute_channels(Image8(pix.data(), w, h, 3 * (int64_t)w, 3), ch);
        const str_er_cand *c0 = str_er_result_plane_cands(r, 0, &n0);
        std::vector<ER> ers((size_t)n0);
        ERs             list;
        for (int32_t i = 0; i < n0; ++i) {
            ER &e = ers[(size_t)i];
            e.bound.x = c0[i].x; e.bound.y = c0[i].y; e.bound.width = c0[i].w; e.bound.height = c0[i].h;
            e.level = c0[i].level; e.key = c0[i].key; e.area = (int)c0[i].area;
            list.push_back(&e);
        }
        const std::vector<str_er_stroke> single = f.er_strokes(Image8(ch[0].data(), w, h, w, 1), list);
        const int32_t first = (int32_t)(c0 - cands);
        bool          same = true;
        for (int32_t i = 0; i < n0 && same; ++i) same = std::memcmp(&single[(size_t)i], &strokes[first + i], sizeof(str_er_stroke)) == 0;
        std::printf("plane 0: %d records, fused == single-stage: %s\n", n0, same ? "yes" : "no");
        return same ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
