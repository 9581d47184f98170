// example_lattice_track.cpp -- every word track of a few consecutive frames matched against a word list over the piece lattices of all
// its members (STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_LINKS | STR_ER_WANT_LINE_WORDS | STR_ER_WANT_RUN_READ | STR_ER_WANT_RUN_SPLIT |
// STR_ER_WANT_WORD_MATCH | STR_ER_WANT_TRACK_READ | STR_ER_WANT_LATTICE_MATCH | STR_ER_WANT_LATTICE_TRACK).
//
//   g++ -std=c++17 -O2 example_lattice_track.cpp -I../../include -L../lib -lstr_er_hip -o example_lattice_track
//   ./example_lattice_track strong.classifier weak.classifier ocr.model words.txt frames.bgr width height n_frames [INS = 64] [DEL = 64] [band = 2]
//
// frames.bgr holds n_frames raw interleaved 8-bit BGR frames of one size back to back, ocr.model is a libsvm model of the 1800 chain-code
// features, words.txt one word a line (1 .. 32 characters of 0-9 A-Z a-z & ( ); other lines are skipped).  Prints one row per word track,
// "<track> frames <first> .. <last> <members> members -> <track match's entry> <cost> | <lattice track entry> <cost> (<used> used,
// <tried> tried)", and under it one row per member, "  word <w>: <reading> cost <own cost>, <runs> runs in <parts> parts, <dropped>
// dropped, <inserted> inserted": the track match's entry is the best of the list on the members' split sequences (str_er_track_match
// beside str_er_run_split), the lattice track entry the best when every member's segmentation is free (the contract is at
// str_er_lattice_track_member in str_er.h).  Costs are in 1/8 bit.
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
    if (argc < 9 || argc > 12) {
        std::fprintf(stderr, "usage: %s strong.classifier weak.classifier ocr.model words.txt frames.bgr width height n_frames [INS] [DEL] [band]\n", argv[0]);
        return 2;
    }
    const int w = std::atoi(argv[6]), h = std::atoi(argv[7]), nf = std::atoi(argv[8]), ins = argc > 9 ? std::atoi(argv[9]) : 64, del = argc > 10 ? std::atoi(argv[10]) : 64,
              band = argc > 11 ? std::atoi(argv[11]) : 2;
    if (w < 1 || h < 1 || nf < 1) { std::fprintf(stderr, "bad size\n"); return 2; }
    std::vector<uint8_t> pix((size_t)w * h * 3 * (size_t)nf);
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
    p.max_width = w; p.max_height = h; p.max_frames = nf; p.n_pyr_levels = 3;
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
    const int rc = str_er_detect_bgr(c, pix.data(), w, h, 3 * (int64_t)w, 3 * (int64_t)w * h, nf, STR_ER_MEM_HOST,
                                     STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_LINKS |
                                         STR_ER_WANT_LINE_WORDS | STR_ER_WANT_RUN_READ | STR_ER_WANT_RUN_SPLIT | STR_ER_WANT_WORD_MATCH | STR_ER_WANT_TRACK_READ |
                                         STR_ER_WANT_LATTICE_MATCH | STR_ER_WANT_LATTICE_TRACK, &r);
    if (rc != STR_ER_OK) { std::fprintf(stderr, "detect: %s\n", str_er_last_error(c)); return 1; }
    std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
    const ERFilter::LineWords           lw = ERFilter::line_words(r);
    const ERFilter::RunReads            rd = ERFilter::run_reads(r);
    const ERFilter::TrackRead           tr = ERFilter::track_read(r);
    const ERFilter::LatticeTrackMatches lt = ERFilter::lattice_track_matches(r);
    for (size_t g = 0; g < tr.tracks.size(); ++g) {
        const str_er_word_track  &T = tr.tracks[g];
        const str_er_track_match &d = lt.matches[g];
        std::printf("%zu frames %u .. %u %d members -> %s %d | %s %d (%d used, %d tried)\n", g, T.first_frame, T.last_frame, T.count,
                    ERFilter::word_track_text(lw, rd, tr, lexicon, g).c_str(), tr.matches[g].cost, ERFilter::word_track_lattice_text(lt, lexicon, g).c_str(), d.cost,
                    d.n_used, d.n_tried);
        for (int32_t i = T.first; i < T.first + T.count; ++i) {
            const str_er_lattice_track_member &M = lt.members[(size_t)i];
            std::printf("  word %d: %s cost %d, %d runs in %d parts, %d dropped, %d inserted\n", M.word, ERFilter::word_text(lw, rd, (size_t)M.word).c_str(), M.cost,
                        lw.words[(size_t)M.word].n_runs, M.n_parts, M.n_del, M.n_ins);
        }
    }
    return 0;
}
