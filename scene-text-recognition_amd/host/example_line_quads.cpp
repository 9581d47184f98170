// example_line_quads.cpp -- the oriented box of every text line of a frame (STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_GEOM).
//
//   g++ -std=c++17 -O2 example_line_quads.cpp -I../../include -L../lib -lstr_er_hip -o example_line_quads
//   ./example_line_quads strong.classifier weak.classifier frame.bgr width height [pyramid levels = 3]
//
// frame.bgr is a raw interleaved 8-bit BGR dump.  Prints one row per frame line, "<frame> <x0> <y0> <x1> <y1> <x2> <y2> <x3> <y3>": the
// four corners of its box in frame pixels, clockwise, the order of an ICDAR incidental-text result file (which rounds them to integers;
// here they are printed exactly, %.17g).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <vector>

#include "er_filter_hip.hpp"

using namespace str_er_host;

int main(int argc, char **argv)
{
    if (argc != 6 && argc != 7) {
        std::fprintf(stderr, "usage: %s strong.classifier weak.classifier frame.bgr width height [pyramid levels]\n", argv[0]);
        return 2;
    }
    const int w = std::atoi(argv[4]), h = std::atoi(argv[5]), levels = argc == 7 ? std::atoi(argv[6]) : 3;
    if (w < 1 || h < 1 || levels < 1) { std::fprintf(stderr, "bad size\n"); return 2; }
    std::vector<uint8_t> pix((size_t)w * h * 3);
    std::ifstream in(argv[3], std::ios::binary);
    if (!in.read(reinterpret_cast<char *>(pix.data()), (std::streamsize)pix.size())) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
    str_er_params p;
    str_er_default_params(&p);
    p.max_width = w; p.max_height = h; p.max_frames = 1; p.n_pyr_levels = levels;
    str_er_ctx *c = nullptr;
    if (str_er_create(&p, &c) != STR_ER_OK) { std::fprintf(stderr, "create: %s\n", str_er_last_error(nullptr)); return 1; }
    std::unique_ptr<str_er_ctx, void (*)(str_er_ctx *)> ctx(c, str_er_destroy);
    if (str_er_load_cascade(c, 0, argv[1]) != STR_ER_OK || str_er_load_cascade(c, 1, argv[2]) != STR_ER_OK) {
        std::fprintf(stderr, "cascades: %s\n", str_er_last_error(c));
        return 1;
    }
    str_er_result *r = nullptr;
    const int rc = str_er_detect_bgr(c, pix.data(), w, h, 3 * (int64_t)w, 3 * (int64_t)w * h, 1, STR_ER_MEM_HOST,
                                     STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_GEOM, &r);
    if (rc != STR_ER_OK) { std::fprintf(stderr, "detect: %s\n", str_er_last_error(c)); return 1; }
    std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
    const ERFilter::FrameLines fl = ERFilter::frame_lines(r);
    const ERFilter::LineGeoms  lg = ERFilter::line_geoms(r);
    for (size_t i = 0; i < lg.frame_lines.size(); ++i) {
        const str_er_line_geom &g = lg.frame_lines[i];
        std::printf("%u", fl.lines[i].frame);
        for (int k = 0; k < 4; ++k) std::printf(" %.17g %.17g", g.qx[k], g.qy[k]);
        std::printf("\n");
    }
    return 0;
}
