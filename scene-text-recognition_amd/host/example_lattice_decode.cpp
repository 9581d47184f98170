// example_lattice_decode.cpp -- every word of a frame decoded jointly over the pieces of its glyph runs and a character bigram table made
// from a word list (STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_WORDS | STR_ER_WANT_RUN_READ | STR_ER_WANT_RUN_SPLIT | STR_ER_WANT_LATTICE_DECODE).
//
//   g++ -std=c++17 -O2 example_lattice_decode.cpp -I../../include -L../lib -lstr_er_hip -o example_lattice_decode
//   ./example_lattice_decode strong.classifier weak.classifier ocr.model words.txt frame.bgr width height [INS = 64] [DEL = 64]
//
// frame.bgr is a raw interleaved 8-bit BGR dump, ocr.model a libsvm model of the 1800 chain-code features, words.txt one word a line
// (characters of 0-9 A-Z a-z & ( ); other lines are skipped).  The table is the add-one bigram counts of the words with the word
// boundary, every row normalised, through str_er_bigram_from_probs.  Prints one row per word of every frame line,
// "<frame> <frame line> <word> <reading> / <split reading> -> <decoded> <cost> (reading <its cost>, <runs> runs in <parts> parts,
// <parts read> read, <dropped> dropped, <inserted> inserted) margins <reading> <cut>": the reading is a character per glyph run, the split reading a character per
// part of the scorer's own segmentation (str_er_run_split), the decoded string the cheapest over every segmentation of the runs into their
// pieces under the pieces' cost rows plus the table (the contract is at str_er_lattice_decode in str_er.h); the margins say how much more the
// cheapest path costs that reads some part differently and that cuts the word differently (str_er_lattice_margin; -1: no run of the word is
// cut, or the word was not decoded).  Costs are in 1/8 bit.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "er_filter_hip.hpp"

using namespace str_er_host;

static int label_of(char ch)
{
    if (ch >= '0' && ch <= '9') return ch - '0';
    if (ch >= 'A' && ch <= 'Z') return 10 + (ch - 'A');
    if (ch >= 'a' && ch <= 'z') return 36 + (ch - 'a');
    return ch == '&' ? 62 : ch == '(' ? 63 : ch == ')' ? 64 : -1;
}

int main(int argc, char **argv)
{
    if (argc < 8 || argc > 10) {
        std::fprintf(stderr, "usage: %s strong.classifier weak.classifier ocr.model words.txt frame.bgr width height [INS] [DEL]\n", argv[0]);
        return 2;
    }
    const int w = std::atoi(argv[6]), h = std::atoi(argv[7]), ins = argc > 8 ? std::atoi(argv[8]) : 64, del = argc > 9 ? std::atoi(argv[9]) : 64;
    if (w < 1 || h < 1) { std::fprintf(stderr, "bad size\n"); return 2; }
    std::vector<uint8_t> pix((size_t)w * h * 3);
    std::ifstream in(argv[5], std::ios::binary);
    if (!in.read(reinterpret_cast<char *>(pix.data()), (std::streamsize)pix.size())) { std::fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    // add-one counts over the 66 symbols, rows normalised
    std::vector<double> cnt(66 * 66, 1.0);
    {
        std::ifstream words(argv[4]);
        for (std::string line; std::getline(words, line);) {
            while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
            bool ok = !line.empty();
            for (const char ch : line) ok = ok && label_of(ch) >= 0;
            if (!ok) continue;
            int prev = 65;
            for (const char ch : line) { cnt[(size_t)prev * 66 + (size_t)label_of(ch)] += 1; prev = label_of(ch); }
            cnt[(size_t)prev * 66 + 65] += 1;
        }
    }
    std::vector<double> tp(65 * 65), start(65), end(65);
    for (int a = 0; a < 66; ++a) {
        double tot = 0;
        for (int b = 0; b < 66; ++b) tot += cnt[(size_t)a * 66 + b];
        for (int b = 0; b < 66; ++b) {
            const double p = cnt[(size_t)a * 66 + b] / tot;
            if (a < 65 && b < 65) tp[(size_t)a * 65 + b] = p;
            else if (a == 65 && b < 65) start[(size_t)b] = p;
            else if (a < 65) end[(size_t)a] = p;
        }
    }
    uint8_t table[66 * 66];
    if (str_er_bigram_from_probs(tp.data(), start.data(), end.data(), table) != STR_ER_OK) return 1;
    str_er_params p;
    str_er_default_params(&p);
    p.max_width = w; p.max_height = h; p.max_frames = 1; p.n_pyr_levels = 3;
    str_er_ctx *c = nullptr;
    if (str_er_create(&p, &c) != STR_ER_OK) { std::fprintf(stderr, "create: %s\n", str_er_last_error(nullptr)); return 1; }
    std::unique_ptr<str_er_ctx, void (*)(str_er_ctx *)> ctx(c, str_er_destroy);
    if (str_er_load_cascade(c, 0, argv[1]) != STR_ER_OK || str_er_load_cascade(c, 1, argv[2]) != STR_ER_OK || str_er_load_svm_model(c, argv[3], 1800) != STR_ER_OK ||
        str_er_set_bigram(c, table) != STR_ER_OK || str_er_set_word_decode(c, ins, del) != STR_ER_OK || str_er_set_lattice_margin(c, 1) != STR_ER_OK) {
        std::fprintf(stderr, "models and table: %s\n", str_er_last_error(c));
        return 1;
    }
    str_er_result *r = nullptr;
    const int rc = str_er_detect_bgr(c, pix.data(), w, h, 3 * (int64_t)w, 3 * (int64_t)w * h, 1, STR_ER_MEM_HOST,
                                     STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_WORDS |
                                         STR_ER_WANT_RUN_READ | STR_ER_WANT_RUN_SPLIT | STR_ER_WANT_LATTICE_DECODE, &r);
    if (rc != STR_ER_OK) { std::fprintf(stderr, "detect: %s\n", str_er_last_error(c)); return 1; }
    std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
    const ERFilter::FrameLines  fl = ERFilter::frame_lines(r);
    const ERFilter::LineWords   lw = ERFilter::line_words(r);
    const ERFilter::RunReads    rd = ERFilter::run_reads(r);
    const ERFilter::RunSplits      sp = ERFilter::run_splits(r);
    const ERFilter::LatticeDecodes ld = ERFilter::lattice_decodes(r);
    const ERFilter::LatticeMargins lg = ERFilter::lattice_margins(r);
    for (size_t i = 0; i < fl.lines.size(); ++i) {
        if (fl.lines[i].rep < 0) continue;
        const str_er_line_words &L = lw.lines[(size_t)fl.lines[i].rep];
        for (int32_t k = L.first_word; k < L.first_word + L.n_words; ++k) {
            const str_er_lattice_decode &d = ld.decodes[(size_t)k];
            std::printf("%u %zu %d %s / %s -> %s %d (reading %d, %d runs in %d parts, %d read, %d dropped, %d inserted) margins %d %d\n", fl.lines[i].frame, i, k - L.first_word,
                        ERFilter::word_text(lw, rd, (size_t)k).c_str(), ERFilter::word_split_text(sp, (size_t)k).c_str(),
                        ERFilter::word_lattice_text(lw, rd, ld, (size_t)k).c_str(), d.cost, d.read_cost, lw.words[(size_t)k].n_runs, d.n_parts, d.n_sub, d.n_del,
                        d.n_ins, lg.margins[(size_t)k].read_margin, lg.margins[(size_t)k].cut_margin);
        }
    }
    return 0;
}
