// example_track_read.cpp -- the words of a short video linked across its frames, and every word track matched against a word list
// over the readings of all its members (STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_LINKS | STR_ER_WANT_LINE_WORDS | STR_ER_WANT_RUN_READ |
// STR_ER_WANT_WORD_MATCH | STR_ER_WANT_TRACK_READ).
//
//   g++ -std=c++17 -O2 example_track_read.cpp -I../../include -L../lib -lstr_er_hip -o example_track_read
//   ./example_track_read strong.classifier weak.classifier ocr.model words.txt frames.bgr width height n_frames [pyramid levels = 3]
//
// frames.bgr holds n_frames raw interleaved 8-bit BGR frames back to back, ocr.model is a libsvm model of the 1800 chain-code features,
// words.txt one word a line (1 .. 32 characters of 0-9 A-Z a-z & ( ); other lines are skipped).  Prints one row per word track,
// "<text track> <word track> frames <first>-<last> <members> members -> <entry> <cost> (second <entry> <cost>, <usable members> used)"
// and under it one row per member, "<frame> <word> <reading> -> <the word's own match> <its cost for the track's entry>": pooled over
// the members, a track can take an entry that no member takes alone (the contract is at str_er_word_link in str_er.h).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "er_filter_hip.hpp"

using namespace str_er_host;

static bool in_alphabet(const std::string &w)
{
    if (w.empty() || w.size() > 32) return false;
    for (const char ch : w)
        if (!((ch >= '0' && ch <= '9') || (ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z') || ch == '&' || ch == '(' || ch == ')')) return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 9 && argc != 10) {
        std::fprintf(stderr, "usage: %s strong.classifier weak.classifier ocr.model words.txt frames.bgr width height n_frames [pyramid levels]\n", argv[0]);
        return 2;
    }
    const int w = std::atoi(argv[6]), h = std::atoi(argv[7]), n_frames = std::atoi(argv[8]), levels = argc == 10 ? std::atoi(argv[9]) : 3;
    if (w < 1 || h < 1 || n_frames < 1 || levels < 1) { std::fprintf(stderr, "bad size\n"); return 2; }
    std::vector<uint8_t> pix((size_t)w * h * 3 * n_frames);
    std::ifstream in(argv[5], std::ios::binary);
    if (!in.read(reinterpret_cast<char *>(pix.data()), (std::streamsize)pix.size())) { std::fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    std::vector<std::string> lexicon;
    std::string              bytes;
    std::vector<int32_t>     offsets{0};
    {
        std::ifstream words(argv[4]);
        for (std::string line; std::getline(words, line) && lexicon.size() < ((size_t)1 << 20);) {
            while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
            if (!in_alphabet(line)) continue;
            lexicon.push_back(line);
            bytes += line;
            offsets.push_back((int32_t)bytes.size());
        }
    }
    if (lexicon.empty()) { std::fprintf(stderr, "no usable word in %s\n", argv[4]); return 2; }
    str_er_params p;
    str_er_default_params(&p);
    p.max_width = w; p.max_height = h; p.max_frames = n_frames; p.n_pyr_levels = levels;
    str_er_ctx *c = nullptr;
    if (str_er_create(&p, &c) != STR_ER_OK) { std::fprintf(stderr, "create: %s\n", str_er_last_error(nullptr)); return 1; }
    std::unique_ptr<str_er_ctx, void (*)(str_er_ctx *)> ctx(c, str_er_destroy);
    if (str_er_load_cascade(c, 0, argv[1]) != STR_ER_OK || str_er_load_cascade(c, 1, argv[2]) != STR_ER_OK || str_er_load_svm_model(c, argv[3], 1800) != STR_ER_OK ||
        str_er_set_lexicon(c, bytes.data(), offsets.data(), (int32_t)lexicon.size(), STR_ER_LEXICON_FOLD_CASE) != STR_ER_OK) {
        std::fprintf(stderr, "models and lexicon: %s\n", str_er_last_error(c));
        return 1;
    }
    str_er_result *r = nullptr;
    const int rc = str_er_detect_bgr(c, pix.data(), w, h, 3 * (int64_t)w, 3 * (int64_t)w * h, n_frames, STR_ER_MEM_HOST,
                                     STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_LINKS |
                                         STR_ER_WANT_LINE_WORDS | STR_ER_WANT_RUN_READ | STR_ER_WANT_WORD_MATCH | STR_ER_WANT_TRACK_READ, &r);
    if (rc != STR_ER_OK) { std::fprintf(stderr, "detect: %s\n", str_er_last_error(c)); return 1; }
    std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
    const ERFilter::LineWords   lw = ERFilter::line_words(r);
    const ERFilter::RunReads    rd = ERFilter::run_reads(r);
    const ERFilter::WordMatches wm = ERFilter::word_matches(r);
    const ERFilter::TrackRead   tr = ERFilter::track_read(r);
    int32_t n_texts = 0;
    const str_er_text *texts = str_er_result_texts(r, &n_texts);
    for (size_t g = 0; g < tr.tracks.size(); ++g) {
        const str_er_word_track  &T = tr.tracks[g];
        const str_er_track_match &m = tr.matches[g];
        std::printf("%d %zu frames %u-%u %d members -> %s %d (second %d %d, %d used)\n", T.text_track, g, T.first_frame, T.last_frame, T.count,
                    ERFilter::word_track_text(lw, rd, tr, lexicon, g).c_str(), m.cost, m.second_entry, m.second_cost, m.n_used);
        for (int32_t k = T.first; k < T.first + T.count; ++k) {
            const size_t  word = (size_t)tr.members[(size_t)k];
            const int32_t line = lw.words[word].line;
            std::printf("    %u %zu %s -> %s %d\n", line >= 0 && line < n_texts ? texts[line].frame : 0u, word, ERFilter::word_text(lw, rd, word).c_str(),
                        ERFilter::word_match_text(lw, rd, wm, lexicon, word).c_str(), tr.member_costs[(size_t)k]);
        }
    }
    return 0;
}
