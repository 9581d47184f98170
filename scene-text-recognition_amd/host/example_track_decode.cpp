// example_track_decode.cpp -- the words of a short video linked across its frames, and every word track decoded without a word list:
// one string per track from the readings of all its members under a character bigram table
// (STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_LINKS | STR_ER_WANT_LINE_WORDS | STR_ER_WANT_RUN_READ | STR_ER_WANT_WORD_DECODE |
// STR_ER_WANT_TRACK_DECODE).
//
//   g++ -std=c++17 -O2 example_track_decode.cpp -I../../include -L../lib -lstr_er_hip -o example_track_decode
//   ./example_track_decode strong.classifier weak.classifier ocr.model text.txt frames.bgr width height n_frames [rounds = 8]
//
// frames.bgr holds n_frames raw interleaved 8-bit BGR frames back to back, ocr.model is a libsvm model of the 1800 chain-code features,
// text.txt any text of the kind the video shows, one word a line (characters of 0-9 A-Z a-z & ( ); other lines are skipped): it only
// trains the table -- the add-one bigram counts with the word boundary, every row normalised, through str_er_bigram_from_probs -- and
// the strings that come out need not be in it.  Prints one row per word track,
// "<text track> <word track> frames <first>-<last> <members> members -> <string> <cost> (set median <its cost> from word <seed>, <edits>
// edits, <converged>, <usable members> used)" and under it one row per member, "<frame> <word> <reading> -> <the word's own decode> <its
// alignment cost for the track's string>" (the contract is at str_er_track_decode in str_er.h).  Costs are in 1/8 bit.
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
    if (argc != 9 && argc != 10) {
        std::fprintf(stderr, "usage: %s strong.classifier weak.classifier ocr.model text.txt frames.bgr width height n_frames [rounds]\n", argv[0]);
        return 2;
    }
    const int w = std::atoi(argv[6]), h = std::atoi(argv[7]), n_frames = std::atoi(argv[8]), rounds = argc == 10 ? std::atoi(argv[9]) : 8;
    if (w < 1 || h < 1 || n_frames < 1) { std::fprintf(stderr, "bad size\n"); return 2; }
    std::vector<uint8_t> pix((size_t)w * h * 3 * n_frames);
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
    p.max_width = w; p.max_height = h; p.max_frames = n_frames; p.n_pyr_levels = 3;
    str_er_ctx *c = nullptr;
    if (str_er_create(&p, &c) != STR_ER_OK) { std::fprintf(stderr, "create: %s\n", str_er_last_error(nullptr)); return 1; }
    std::unique_ptr<str_er_ctx, void (*)(str_er_ctx *)> ctx(c, str_er_destroy);
    if (str_er_load_cascade(c, 0, argv[1]) != STR_ER_OK || str_er_load_cascade(c, 1, argv[2]) != STR_ER_OK || str_er_load_svm_model(c, argv[3], 1800) != STR_ER_OK ||
        str_er_set_bigram(c, table) != STR_ER_OK || str_er_set_track_decode(c, 64, 64, rounds) != STR_ER_OK) {
        std::fprintf(stderr, "models and table: %s\n", str_er_last_error(c));
        return 1;
    }
    str_er_result *r = nullptr;
    const int rc = str_er_detect_bgr(c, pix.data(), w, h, 3 * (int64_t)w, 3 * (int64_t)w * h, n_frames, STR_ER_MEM_HOST,
                                     STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_LINKS |
                                         STR_ER_WANT_LINE_WORDS | STR_ER_WANT_RUN_READ | STR_ER_WANT_WORD_DECODE | STR_ER_WANT_TRACK_DECODE, &r);
    if (rc != STR_ER_OK) { std::fprintf(stderr, "detect: %s\n", str_er_last_error(c)); return 1; }
    std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
    const ERFilter::LineWords    lw = ERFilter::line_words(r);
    const ERFilter::RunReads     rd = ERFilter::run_reads(r);
    const ERFilter::WordDecodes  wd = ERFilter::word_decodes(r);
    const ERFilter::TrackRead    tr = ERFilter::track_read(r);          // (the links and tracks; no matches without STR_ER_WANT_TRACK_READ)
    const ERFilter::TrackDecodes td = ERFilter::track_decodes(r);
    int32_t n_texts = 0;
    const str_er_text *texts = str_er_result_texts(r, &n_texts);
    for (size_t g = 0; g < tr.tracks.size(); ++g) {
        const str_er_word_track   &T = tr.tracks[g];
        const str_er_track_decode &d = td.decodes[g];
        std::printf("%d %zu frames %u-%u %d members -> %s %d (set median %d from word %d, %d edits, %s, %d used)\n", T.text_track, g, T.first_frame, T.last_frame,
                    T.count, ERFilter::word_track_decode_text(lw, rd, tr, td, g).c_str(), d.cost, d.seed_cost, d.seed_member, d.n_edits,
                    d.converged ? "converged" : "not converged", d.n_used);
        for (int32_t k = T.first; k < T.first + T.count; ++k) {
            const size_t  word = (size_t)tr.members[(size_t)k];
            const int32_t line = lw.words[word].line;
            std::printf("    %u %zu %s -> %s %d\n", line >= 0 && line < n_texts ? texts[line].frame : 0u, word, ERFilter::word_text(lw, rd, word).c_str(),
                        ERFilter::word_decode_text(lw, rd, wd, word).c_str(), td.member_costs[(size_t)k]);
        }
    }
    return 0;
}
