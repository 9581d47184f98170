// words_host.cpp -- the C ABI, part 8b: the words of text lines from their glyph runs (str_er_words_from_runs; the contract is at
// str_er_line_run in str_er.h), the character of a label (str_er_ocr_char) and the shelf packer of the run tiles' atlas
// (pack_run_tiles; STR_ER_WANT_RUN_READ).  Pure host and HIP-free: it includes nothing of the library but the public header and the
// plain structures of er_types.h, so that tests/cpp/line_words_rules_check.cpp and run_read_rules_check.cpp link this file alone
// under the host sanitizers.  The detect calls, str_er_feet_words (api_frame_lines.cpp) and str_er_feet_read (api_run_read.cpp) use
// these same functions.  lines_host.cpp holds the rest of the line stage's host code in the same way.
#include "../../include/str_er.h"
#include "er_types.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace str_er_host {

// the num / den str_er_set_word_gap and str_er_words_from_runs take (g * den and num * colmax then stay far below 2^63)
bool word_gap_ok(int32_t num, int32_t den) { return num >= 1 && num <= 65535 && den >= 1 && den <= 65535; }

} // namespace str_er_host

namespace str_er {

bool pack_run_tiles(RunTile *tiles, size_t n, uint32_t shelf_w, RunAtlas &atlas)
{
    atlas = RunAtlas{0, 0};
    if (n == 0) return true;
    uint64_t width = (shelf_w + 3u) / 4u * 4u;
    for (size_t k = 0; k < n; ++k) {
        if (tiles[k].w == 0 || tiles[k].h == 0) return false;
        width = std::max<uint64_t>(width, ((uint64_t)tiles[k].w + 3u) / 4u * 4u);
    }
    uint64_t x = 0, y = 0, shelf_h = 0;
    for (size_t k = 0; k < n; ++k) {
        const uint64_t w4 = ((uint64_t)tiles[k].w + 3u) / 4u * 4u;
        if (x + w4 > width) { y += shelf_h; x = 0; shelf_h = 0; }         // (the shelf is full: the next one)
        tiles[k].ax = (uint32_t)x; tiles[k].ay = (uint32_t)y;
        x += w4;
        shelf_h = std::max<uint64_t>(shelf_h, tiles[k].h);
        if (y + shelf_h > 0x7FFFFFFFull) return false;
    }
    atlas.width = (uint32_t)width; atlas.height = (uint32_t)(y + shelf_h);
    return true;
}

} // namespace str_er

extern "C" {

int32_t str_er_ocr_char(int32_t label)
{
    static const char table[] = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz&()";        // src/OCR.cpp:10
    static_assert(sizeof(table) == 66, "65 characters");
    return label >= 0 && label < 65 ? (int32_t)table[label] : (int32_t)'?';
}

int str_er_words_from_runs(str_er_line_run *runs, int32_t n_runs, str_er_line_words *line_words, int32_t n_lines, int32_t num, int32_t den,
                           str_er_line_word *words, int32_t cap_words, int32_t *n_words)
try {
    if (n_runs < 0 || n_lines < 0 || !n_words || !str_er_host::word_gap_ok(num, den)) return STR_ER_EINVAL;
    if ((n_runs > 0 && !runs) || (n_lines > 0 && !line_words) || (words && cap_words < 0)) return STR_ER_EINVAL;
    // the run lists back to back, every run a run and every gap a gap, before anything is written
    int64_t at = 0;
    for (int32_t t = 0; t < n_lines; ++t) {
        const str_er_line_words &LW = line_words[t];
        if (LW.n_runs < 0 || LW.first_run != at || at + LW.n_runs > n_runs || (LW.n_runs > 0 && LW.colmax == 0)) return STR_ER_EINVAL;
        for (int32_t k = 0; k < LW.n_runs; ++k) {
            const str_er_line_run &R = runs[at + k];
            if (R.x0 >= R.x1 || R.y0 >= R.y1 || R.pixels == 0 || (k > 0 && R.x0 <= runs[at + k - 1].x1)) return STR_ER_EINVAL;
        }
        at += LW.n_runs;
    }
    if (at != n_runs) return STR_ER_EINVAL;
    std::vector<str_er_line_word> out;
    for (int32_t t = 0; t < n_lines; ++t) {
        str_er_line_words &LW = line_words[t];
        LW.first_word = (int32_t)out.size(); LW.reserved = 0;
        for (int32_t k = 0; k < LW.n_runs; ++k) {
            str_er_line_run &R = runs[LW.first_run + k];
            const bool brk = k == 0 || (uint64_t)((int64_t)R.x0 - runs[LW.first_run + k - 1].x1) * (uint64_t)den >= (uint64_t)num * (uint64_t)LW.colmax;
            if (brk) {
                if (out.size() >= 0x7FFFFFFFull) return STR_ER_ECAPACITY;
                out.push_back(str_er_line_word{t, LW.first_run + k, 0, R.x0, R.y0, 0, 0, 0});
            }
            str_er_line_word &Wd = out.back();
            const int32_t y1 = std::max(Wd.y + Wd.h, R.y1);         // (h is 0 for a word just begun: y1 = R.y1 > R.y0)
            Wd.y = std::min(Wd.y, R.y0); Wd.h = y1 - Wd.y;
            Wd.w = R.x1 - Wd.x;
            Wd.pixels += R.pixels; ++Wd.n_runs;
            R.word = (int32_t)out.size() - 1;
        }
        LW.n_words = (int32_t)out.size() - LW.first_word;
    }
    *n_words = (int32_t)out.size();
    if (!words) return STR_ER_OK;
    if ((int64_t)out.size() > (int64_t)cap_words) return STR_ER_ECAPACITY;
    if (!out.empty()) std::memcpy(words, out.data(), sizeof(str_er_line_word) * out.size());
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

} // extern "C"
