// words_host.cpp -- the C ABI, part 8b: the words of text lines from their glyph runs (str_er_words_from_runs; the contract is at
// str_er_line_run in str_er.h).  Pure host and HIP-free: it includes nothing of the library but the public header, so that
// tests/cpp/line_words_rules_check.cpp links this file alone under the host sanitizers.  The detect calls and str_er_feet_words
// (api_frame_lines.cpp) form their words with this same function.
#include "../../include/str_er.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace str_er_host {

// the num / den str_er_set_word_gap and str_er_words_from_runs take (g * den and num * colmax then stay far below 2^63)
bool word_gap_ok(int32_t num, int32_t den) { return num >= 1 && num <= 65535 && den >= 1 && den <= 65535; }

} // namespace str_er_host

extern "C" {

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
