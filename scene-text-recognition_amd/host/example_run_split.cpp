// example_run_split.cpp -- the touching glyphs of a frame split: every glyph run cut at the valleys of its column profile, the pieces
// read, and per word the split sequence the scorer likes best
// (STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_WORDS | STR_ER_WANT_RUN_READ | STR_ER_WANT_RUN_SPLIT).
//
//   g++ -std=c++17 -O2 example_run_split.cpp -I../../include -L../lib -lstr_er_hip -o example_run_split
//   ./example_run_split strong.classifier weak.classifier ocr.model frame.bgr width height [num = 1] [den = 4] [SPLIT = 8]
//
// frame.bgr is a raw interleaved 8-bit BGR dump, ocr.model a libsvm model of the 1800 chain-code features.  A column of a run is low at
// floor(height * num / den) pixels or fewer; a split pays SPLIT (1/8 bit).  Prints one row per word of every frame line,
// "<frame> <frame line> <word> <reading> -> <split reading> <parts> parts of <runs> runs, cost <cost> (reading <its cost>)", and under
// it one row per cut run of the word, "  run <run> [<x0>, <x1>) cut at <columns>: <parts of the run>".  The contract is at
// str_er_run_split in str_er.h.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "er_filter_hip.hpp"

using namespace str_er_host;

int main(int argc, char **argv)
{
    if (argc < 7 || argc > 10) {
        std::fprintf(stderr, "usage: %s strong.classifier weak.classifier ocr.model frame.bgr width height [num] [den] [SPLIT]\n", argv[0]);
        return 2;
    }
    const int w = std::atoi(argv[5]), h = std::atoi(argv[6]);
    const int num = argc > 7 ? std::atoi(argv[7]) : 1, den = argc > 8 ? std::atoi(argv[8]) : 4, split = argc > 9 ? std::atoi(argv[9]) : 8;
    if (w < 1 || h < 1) { std::fprintf(stderr, "bad size\n"); return 2; }
    std::vector<uint8_t> pix((size_t)w * h * 3);
    std::ifstream in(argv[4], std::ios::binary);
    if (!in.read(reinterpret_cast<char *>(pix.data()), (std::streamsize)pix.size())) { std::fprintf(stderr, "cannot read %s\n", argv[4]); return 2; }
    str_er_params p;
    str_er_default_params(&p);
    p.max_width = w; p.max_height = h; p.max_frames = 1; p.n_pyr_levels = 3;
    str_er_ctx *c = nullptr;
    if (str_er_create(&p, &c) != STR_ER_OK) { std::fprintf(stderr, "create: %s\n", str_er_last_error(nullptr)); return 1; }
    std::unique_ptr<str_er_ctx, void (*)(str_er_ctx *)> ctx(c, str_er_destroy);
    if (str_er_load_cascade(c, 0, argv[1]) != STR_ER_OK || str_er_load_cascade(c, 1, argv[2]) != STR_ER_OK || str_er_load_svm_model(c, argv[3], 1800) != STR_ER_OK ||
        str_er_set_run_split(c, num, den, split) != STR_ER_OK) {
        std::fprintf(stderr, "models and parameters: %s\n", str_er_last_error(c));
        return 1;
    }
    str_er_result *r = nullptr;
    const int rc = str_er_detect_bgr(c, pix.data(), w, h, 3 * (int64_t)w, 3 * (int64_t)w * h, 1, STR_ER_MEM_HOST,
                                     STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_WORDS |
                                         STR_ER_WANT_RUN_READ | STR_ER_WANT_RUN_SPLIT, &r);
    if (rc != STR_ER_OK) { std::fprintf(stderr, "detect: %s\n", str_er_last_error(c)); return 1; }
    std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
    const ERFilter::FrameLines fl = ERFilter::frame_lines(r);
    const ERFilter::LineWords  lw = ERFilter::line_words(r);
    const ERFilter::RunReads   rd = ERFilter::run_reads(r);
    const ERFilter::RunSplits  sp = ERFilter::run_splits(r);
    for (size_t i = 0; i < fl.lines.size(); ++i) {
        if (fl.lines[i].rep < 0) continue;
        const str_er_line_words &L = lw.lines[(size_t)fl.lines[i].rep];
        for (int32_t k = L.first_word; k < L.first_word + L.n_words; ++k) {
            const str_er_line_word  &W = lw.words[(size_t)k];
            const str_er_word_split &S = sp.word_splits[(size_t)k];
            std::printf("%u %zu %d %s -> %s %d parts of %d runs, cost %d (reading %d)\n", fl.lines[i].frame, i, k - L.first_word,
                        ERFilter::word_text(lw, rd, (size_t)k).c_str(), ERFilter::word_split_text(sp, (size_t)k).c_str(), S.n_parts, W.n_runs, S.cost, S.read_cost);
            for (int32_t q = W.first_run; q < W.first_run + W.n_runs; ++q) {
                const str_er_run_split &C = sp.splits[(size_t)q];
                if (C.n_cuts == 0) continue;
                std::printf("  run %d [%d, %d) cut at", q, lw.runs[(size_t)q].x0, lw.runs[(size_t)q].x1);
                for (int32_t t = 0; t < C.n_cuts; ++t) std::printf(" %d", C.cut[t]);
                std::printf(": %d parts\n", C.n_parts);
            }
        }
    }
    return 0;
}
