// example_line_words.cpp -- the word boxes of every text line of a frame (STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_WORDS).
//
//   g++ -std=c++17 -O2 example_line_words.cpp -I../../include -L../lib -lstr_er_hip -o example_line_words
//   ./example_line_words strong.classifier weak.classifier frame.bgr width height [pyramid levels = 3]
//
// frame.bgr is a raw interleaved 8-bit BGR dump.  Prints one row per word of every frame line (the words of its representative line),
// "<frame> <frame line> <x0> <y0> <x1> <y1> <runs>": the word's box in frame pixels, half open, as an ICDAR word box wants it, and the number of
// glyph runs in it.
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
                                     STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_WORDS, &r);
    if (rc != STR_ER_OK) { std::fprintf(stderr, "detect: %s\n", str_er_last_error(c)); return 1; }
    std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
    const ERFilter::FrameLines fl = ERFilter::frame_lines(r);
    const ERFilter::LineWords  lw = ERFilter::line_words(r);
    for (size_t i = 0; i < fl.lines.size(); ++i) {
        if (fl.lines[i].rep < 0) continue;
        const str_er_line_words &L = lw.lines[(size_t)fl.lines[i].rep];
        for (int32_t k = L.first_word; k < L.first_word + L.n_words; ++k) {
            const str_er_line_word &W = lw.words[(size_t)k];
            std::printf("%u %zu %d %d %d %d %d\n", fl.lines[i].frame, i, W.x, W.y, W.x + W.w, W.y + W.h, W.n_runs);
        }
    }
    return 0;
}
