// example_lattice_match.cpp -- every word of a frame matched against a word list with the segmentation of its glyph runs free
// (STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_WORDS | STR_ER_WANT_RUN_READ | STR_ER_WANT_RUN_SPLIT | STR_ER_WANT_WORD_MATCH |
// STR_ER_WANT_LATTICE_MATCH).
//
//   g++ -std=c++17 -O2 example_lattice_match.cpp -I../../include -L../lib -lstr_er_hip -o example_lattice_match
//   ./example_lattice_match strong.classifier weak.classifier ocr.model words.txt frame.bgr width height [INS = 64] [DEL = 64] [band = 2]
//
// frame.bgr is a raw interleaved 8-bit BGR dump, ocr.model a libsvm model of the 1800 chain-code features, words.txt one word a line
// (1 .. 32 characters of 0-9 A-Z a-z & ( ); other lines are skipped).  Prints one row per word of every frame line,
// "<frame> <frame line> <word> <reading> / <split reading> -> <matcher's entry> <cost> | <lattice entry> <cost> (<runs> runs in <parts>
// parts, <dropped> dropped, <inserted> inserted, <tried> tried)": the matcher's entry is the best of the list on the scorer's own
// segmentation (str_er_word_match beside str_er_run_split), the lattice entry the best over every segmentation of the runs into their
// pieces (the contract is at str_er_lattice_match in str_er.h).  Costs are in 1/8 bit.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "er_filter_hip.hpp"

using namespace str_er_host;

static bool in_alphabet(char ch)
{
    return (ch >= '0' && ch <= '9') || (ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z') || ch == '&' || ch == '(' || ch == ')';
}

int main(int argc, char **argv)
{
    if (argc < 8 || argc > 11) {
        std::fprintf(stderr, "usage: %s strong.classifier weak.classifier ocr.model words.txt frame.bgr width height [INS] [DEL] [band]\n", argv[0]);
        return 2;
    }
    const int w = std::atoi(argv[6]), h = std::atoi(argv[7]), ins = argc > 8 ? std::atoi(argv[8]) : 64, del = argc > 9 ? std::atoi(argv[9]) : 64,
              band = argc > 10 ? std::atoi(argv[10]) : 2;
    if (w < 1 || h < 1) { std::fprintf(stderr, "bad size\n"); return 2; }
    std::vector<uint8_t> pix((size_t)w * h * 3);
    std::ifstream in(argv[5], std::ios::binary);
    if (!in.read(reinterpret_cast<char *>(pix.data()), (std::streamsize)pix.size())) { std::fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    std::vector<std::string> lexicon;
    std::string              bytes;
    std::vector<int32_t>     offsets{0};
    {
        std::ifstream words(argv[4]);
        for (std::string line; std::getline(words, line);) {
            while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
            bool ok = !line.empty() && line.size() <= 32;
            for (const char ch : line) ok = ok && in_alphabet(ch);
            if (!ok) continue;
            lexicon.push_back(line);
            bytes += line;
            offsets.push_back((int32_t)bytes.size());
        }
    }
    str_er_params p;
    str_er_default_params(&p);
    p.max_width = w; p.max_height = h; p.max_frames = 1; p.n_pyr_levels = 3;
    str_er_ctx *c = nullptr;
    if (str_er_create(&p, &c) != STR_ER_OK) { std::fprintf(stderr, "create: %s\n", str_er_last_error(nullptr)); return 1; }
    std::unique_ptr<str_er_ctx, void (*)(str_er_ctx *)> ctx(c, str_er_destroy);
    if (str_er_load_cascade(c, 0, argv[1]) != STR_ER_OK || str_er_load_cascade(c, 1, argv[2]) != STR_ER_OK || str_er_load_svm_model(c, argv[3], 1800) != STR_ER_OK ||
        str_er_set_lexicon(c, bytes.data(), offsets.data(), (int32_t)lexicon.size(), STR_ER_LEXICON_FOLD_CASE) != STR_ER_OK ||
        str_er_set_word_match(c, ins, del, band) != STR_ER_OK) {
        std::fprintf(stderr, "models and lexicon: %s\n", str_er_last_error(c));
        return 1;
    }
    str_er_result *r = nullptr;
    const int rc = str_er_detect_bgr(c, pix.data(), w, h, 3 * (int64_t)w, 3 * (int64_t)w * h, 1, STR_ER_MEM_HOST,
                                     STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_WORDS |
                                         STR_ER_WANT_RUN_READ | STR_ER_WANT_RUN_SPLIT | STR_ER_WANT_WORD_MATCH | STR_ER_WANT_LATTICE_MATCH, &r);
    if (rc != STR_ER_OK) { std::fprintf(stderr, "detect: %s\n", str_er_last_error(c)); return 1; }
    std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
    const ERFilter::FrameLines     fl = ERFilter::frame_lines(r);
    const ERFilter::LineWords      lw = ERFilter::line_words(r);
    const ERFilter::RunReads       rd = ERFilter::run_reads(r);
    const ERFilter::RunSplits      sp = ERFilter::run_splits(r);
    const ERFilter::WordMatches    wm = ERFilter::word_matches(r);
    const ERFilter::LatticeMatches lm = ERFilter::lattice_matches(r);
    for (size_t i = 0; i < fl.lines.size(); ++i) {
        if (fl.lines[i].rep < 0) continue;
        const str_er_line_words &L = lw.lines[(size_t)fl.lines[i].rep];
        for (int32_t k = L.first_word; k < L.first_word + L.n_words; ++k) {
            const str_er_lattice_match &d = lm.matches[(size_t)k];
            std::printf("%u %zu %d %s / %s -> %s %d | %s %d (%d runs in %d parts, %d dropped, %d inserted, %d tried)\n", fl.lines[i].frame, i, k - L.first_word,
                        ERFilter::word_text(lw, rd, (size_t)k).c_str(), ERFilter::word_split_text(sp, (size_t)k).c_str(),
                        ERFilter::word_match_text(lw, rd, wm, lexicon, (size_t)k).c_str(), wm.matches[(size_t)k].cost,
                        ERFilter::word_lattice_match_text(lw, rd, lm, lexicon, (size_t)k).c_str(), d.cost, lw.words[(size_t)k].n_runs, d.n_parts, d.n_del, d.n_ins,
                        d.n_tried);
        }
    }
    return 0;
}
