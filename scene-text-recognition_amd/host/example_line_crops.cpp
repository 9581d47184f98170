// example_line_crops.cpp -- detect the text lines of a frame and write a recogniser-ready crop of each (STR_ER_WANT_LINE_CROPS /
// _GLYPHS) as PGM; then the same grey crops through ERFilter::text_crops, the single-stage form on the host Y plane.
//
//   g++ -std=c++17 -O2 example_line_crops.cpp -I../../include -L../lib -lstr_er_hip -o example_line_crops
//   ./example_line_crops strong.classifier weak.classifier frame.bgr width height out_dir
//
// frame.bgr is a raw interleaved 8-bit BGR dump.  Writes out_dir/line_<t>.pgm (grey) and out_dir/glyph_<t>.pgm for every line of the
// call, prints "line <t> <width> <height> <byte sum>" per line, then whether the fused and the single-stage grey crops agree byte for byte.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>

#include "er_filter_hip.hpp"

using namespace str_er_host;

static bool write_pgm(const std::string &path, const uint8_t *pix, int w, int h)
{
    std::ofstream out(path, std::ios::binary);
    out << "P5\n" << w << " " << h << "\n255\n";
    out.write(reinterpret_cast<const char *>(pix), (std::streamsize)w * h);
    return (bool)out;
}

int main(int argc, char **argv)
{
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s strong.classifier weak.classifier frame.bgr width height out_dir\n", argv[0]);
        return 2;
    }
    const int w = std::atoi(argv[4]), h = std::atoi(argv[5]);
    if (w < 1 || h < 1) { std::fprintf(stderr, "bad size\n"); return 2; }
    const std::string dir = argv[6];
    std::vector<uint8_t> pix((size_t)w * h * 3);
    std::ifstream in(argv[3], std::ios::binary);
    if (!in.read(reinterpret_cast<char *>(pix.data()), (std::streamsize)pix.size())) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
    try {
        ERFilter f(8, 120, 900000, 2, 0.7, 0.15, w, h, 1);
        f.set_stc(argv[1]);
        f.set_wtc(argv[2]);
        str_er_result *r = nullptr;
        const uint32_t stages = STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_WANT_LINE_CROPS | STR_ER_WANT_LINE_GLYPHS;
        int rc = str_er_detect_bgr(f.handle(), pix.data(), w, h, 3 * (int64_t)w, 3 * (int64_t)w * h, 1, STR_ER_MEM_HOST, stages, &r);
        if (rc != STR_ER_OK) { std::fprintf(stderr, "detect: %s\n", str_er_last_error(f.handle())); return 1; }
        std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
        int32_t                 n_text = 0, n_crop = 0, n_ers = 0, n_gb = 0;
        uint64_t                n_grey = 0, n_glyph = 0;
        const str_er_text      *texts = str_er_result_texts(r, &n_text);
        const int32_t          *members = str_er_result_text_ers(r, &n_ers);
        const str_er_gbound    *gb = str_er_result_group_bounds(r, &n_gb);
        const str_er_line_crop *crops = str_er_result_line_crops(r, &n_crop);
        const uint8_t          *grey = str_er_result_line_crop_pixels(r, &n_grey);
        const uint8_t          *glyph = str_er_result_line_glyph_pixels(r, &n_glyph);
        if (!crops || !grey || !glyph || n_crop != n_text) { std::fprintf(stderr, "no line crops\n"); return 1; }
        for (int32_t t = 0; t < n_crop; ++t) {
            const str_er_line_crop &g = crops[t];
            uint64_t sum = 0;
            for (uint64_t k = 0; k < (uint64_t)g.width * g.height; ++k) sum += grey[g.pix_off + k];
            std::printf("line %d %d %d %llu\n", t, g.width, g.height, (unsigned long long)sum);
            if (!write_pgm(dir + "/line_" + std::to_string(t) + ".pgm", grey + g.pix_off, g.width, g.height) ||
                !write_pgm(dir + "/glyph_" + std::to_string(t) + ".pgm", glyph + g.pix_off, g.width, g.height)) {
                std::fprintf(stderr, "cannot write to %s\n", dir.c_str());
                return 1;
            }
        }
        // the same lines through the single-stage call on the Y plane compute_channels gives (one frame, one pyramid level)
        std::vector<std::vector<uint8_t>> ch;
        f.compute_channels(Image8(pix.data(), w, h, 3 * (int64_t)w, 3), ch);
        std::vector<ER>   ers((size_t)n_ers);
        std::vector<Text> lines((size_t)n_text);
        for (int32_t t = 0; t < n_text; ++t)
            for (int32_t k = texts[t].first; k < texts[t].first + texts[t].count; ++k) {
                const str_er_gbound &b = gb[members[k]];
                ER &e = ers[(size_t)k];
                e.bound.x = b.x; e.bound.y = b.y; e.bound.width = b.w; e.bound.height = b.h;
                lines[(size_t)t].ers.push_back(&e);
                lines[(size_t)t].slope = texts[t].slope;
            }
        const std::vector<ERFilter::LineCrop> single = f.text_crops(Image8(ch[0].data(), w, h, w, 1), lines);
        bool same = single.size() == (size_t)n_crop;
        for (int32_t t = 0; t < n_crop && same; ++t) {
            const str_er_line_crop &g = crops[t], &s = single[(size_t)t].geom;
            same = g.width == s.width && g.height == s.height && g.ax == s.ax && g.ay == s.ay && g.ux == s.ux && g.uy == s.uy && g.vx == s.vx && g.vy == s.vy &&
                   std::equal(single[(size_t)t].pixels.begin(), single[(size_t)t].pixels.end(), grey + g.pix_off);
        }
        std::printf("%d lines, fused == single-stage: %s\n", n_crop, same ? "yes" : "no");
        return same ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
