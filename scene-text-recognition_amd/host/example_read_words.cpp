// example_read_words.cpp -- the text of every frame line of a frame (STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_WORDS | STR_ER_WANT_RUN_READ).
//
//   g++ -std=c++17 -O2 example_read_words.cpp -I../../include -L../lib -lstr_er_hip -o example_read_words
//   ./example_read_words strong.classifier weak.classifier ocr.model frame.bgr width height [pyramid levels = 3]
//
// frame.bgr is a raw interleaved 8-bit BGR dump, ocr.model a libsvm model of the 1800 chain-code features.  Prints one row per frame line,
// "<frame> <frame line> <lowest probability of its runs> <text>": the words of its representative line, a character per glyph run, joined by
// blanks.  Nothing is corrected: there is no language model, and touching glyphs read as one character.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <vector>

#include "er_filter_hip.hpp"

using namespace str_er_host;

int main(int argc, char **argv)
{
    if (argc != 7 && argc != 8) {
        std::fprintf(stderr, "usage: %s strong.classifier weak.classifier ocr.model frame.bgr width height [pyramid levels]\n", argv[0]);
        return 2;
    }
    const int w = std::atoi(argv[5]), h = std::atoi(argv[6]), levels = argc == 8 ? std::atoi(argv[7]) : 3;
    if (w < 1 || h < 1 || levels < 1) { std::fprintf(stderr, "bad size\n"); return 2; }
    std::vector<uint8_t> pix((size_t)w * h * 3);
    std::ifstream in(argv[4], std::ios::binary);
    if (!in.read(reinterpret_cast<char *>(pix.data()), (std::streamsize)pix.size())) { std::fprintf(stderr, "cannot read %s\n", argv[4]); return 2; }
    str_er_params p;
    str_er_default_params(&p);
    p.max_width = w; p.max_height = h; p.max_frames = 1; p.n_pyr_levels = levels;
    str_er_ctx *c = nullptr;
    if (str_er_create(&p, &c) != STR_ER_OK) { std::fprintf(stderr, "create: %s\n", str_er_last_error(nullptr)); return 1; }
    std::unique_ptr<str_er_ctx, void (*)(str_er_ctx *)> ctx(c, str_er_destroy);
    if (str_er_load_cascade(c, 0, argv[1]) != STR_ER_OK || str_er_load_cascade(c, 1, argv[2]) != STR_ER_OK || str_er_load_svm_model(c, argv[3], 1800) != STR_ER_OK) {
        std::fprintf(stderr, "models: %s\n", str_er_last_error(c));
        return 1;
    }
    str_er_result *r = nullptr;
    const int rc = str_er_detect_bgr(c, pix.data(), w, h, 3 * (int64_t)w, 3 * (int64_t)w * h, 1, STR_ER_MEM_HOST,
                                     STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_WORDS |
                                         STR_ER_WANT_RUN_READ, &r);
    if (rc != STR_ER_OK) { std::fprintf(stderr, "detect: %s\n", str_er_last_error(c)); return 1; }
    std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
    const ERFilter::FrameLines fl = ERFilter::frame_lines(r);
    const ERFilter::LineWords  lw = ERFilter::line_words(r);
    const ERFilter::RunReads   rd = ERFilter::run_reads(r);
    for (size_t i = 0; i < fl.lines.size(); ++i) {
        if (fl.lines[i].rep < 0) continue;
        const str_er_line_words &L = lw.lines[(size_t)fl.lines[i].rep];
        double lowest = 1.0;
        for (int32_t k = L.first_run; k < L.first_run + L.n_runs; ++k) lowest = std::min(lowest, rd.reads[(size_t)k].prob);
        std::printf("%u %zu %.3f %s\n", fl.lines[i].frame, i, lowest, ERFilter::line_text(lw, rd, (size_t)fl.lines[i].rep).c_str());
    }
    return 0;
}
