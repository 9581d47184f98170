// Host-only check of str_er_words_from_runs (csrc/words_host.cpp, compiled with it under -fsanitize=address,undefined and run by
// tests/test_line_words_host_cpp.py): hand-made cases with their words written out, the break rule at its edges, the error cases,
// and random run lists against a plain restatement of the contract at str_er_line_run.  Every array is sized exactly, so that a
// read or a write past an end is the sanitizer's to find.
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "../../include/str_er.h"

namespace str_er_host { bool word_gap_ok(int32_t num, int32_t den); }

namespace {

long bad = 0, cases = 0;

void expect(bool ok, const char *what, long k = -1)
{
    ++cases;
    if (ok) return;
    if (++bad <= 10) printf("WRONG: %s (%ld)\n", what, k);
}

struct Line { uint32_t colmax; std::vector<str_er_line_run> runs; };

str_er_line_run run(int32_t x0, int32_t x1, int32_t y0, int32_t y1, uint32_t px) { return str_er_line_run{x0, x1, y0, y1, px, -9}; }

// the tables of the call, sized exactly
struct Call {
    std::vector<str_er_line_run>   runs;
    std::vector<str_er_line_words> lw;
    std::vector<str_er_line_word>  words;
    int32_t n_words = -1;
    int     rc = 0;
};

Call call(const std::vector<Line> &lines, int32_t num, int32_t den, int32_t cap = -1)
{
    Call c;
    for (const Line &L : lines) {
        c.lw.push_back(str_er_line_words{-3, -3, (int32_t)c.runs.size(), (int32_t)L.runs.size(), L.colmax, 77u});
        c.runs.insert(c.runs.end(), L.runs.begin(), L.runs.end());
    }
    // first the count, then the words into exactly as many records (or `cap`)
    c.rc = str_er_words_from_runs(c.runs.empty() ? nullptr : c.runs.data(), (int32_t)c.runs.size(), c.lw.empty() ? nullptr : c.lw.data(), (int32_t)c.lw.size(),
                                  num, den, nullptr, 0, &c.n_words);
    if (c.rc != STR_ER_OK) return c;
    c.words.resize((size_t)(cap >= 0 ? cap : c.n_words));
    c.rc = str_er_words_from_runs(c.runs.empty() ? nullptr : c.runs.data(), (int32_t)c.runs.size(), c.lw.empty() ? nullptr : c.lw.data(), (int32_t)c.lw.size(),
                                  num, den, c.words.empty() ? nullptr : c.words.data(), (int32_t)c.words.size(), &c.n_words);
    return c;
}

// the contract, restated: the words of the lines, one by one
void restate(const std::vector<Line> &lines, int32_t num, int32_t den, std::vector<str_er_line_word> &words, std::vector<int32_t> &word_of)
{
    words.clear(); word_of.clear();
    int32_t first = 0;
    for (size_t t = 0; t < lines.size(); ++t) {
        const std::vector<str_er_line_run> &R = lines[t].runs;
        for (size_t k = 0; k < R.size(); ++k) {
            const bool brk = k == 0 || (int64_t)(R[k].x0 - R[k - 1].x1) * den >= (int64_t)num * (int64_t)lines[t].colmax;
            if (brk) words.push_back(str_er_line_word{(int32_t)t, first + (int32_t)k, 0, R[k].x0, R[k].y0, 0, R[k].y1 - R[k].y0, 0});
            str_er_line_word &W = words.back();
            const int32_t y1 = W.y + W.h > R[k].y1 ? W.y + W.h : R[k].y1;
            if (R[k].y0 < W.y) W.y = R[k].y0;
            W.h = y1 - W.y; W.w = R[k].x1 - W.x; W.pixels += R[k].pixels; ++W.n_runs;
            word_of.push_back((int32_t)words.size() - 1);
        }
        first += (int32_t)R.size();
    }
}

bool same_word(const str_er_line_word &a, const str_er_line_word &b)
{
    return a.line == b.line && a.first_run == b.first_run && a.n_runs == b.n_runs && a.x == b.x && a.y == b.y && a.w == b.w && a.h == b.h && a.pixels == b.pixels;
}

void agree(const std::vector<Line> &lines, int32_t num, int32_t den, long k)
{
    std::vector<str_er_line_word> words;
    std::vector<int32_t> word_of;
    restate(lines, num, den, words, word_of);
    const Call c = call(lines, num, den);
    expect(c.rc == STR_ER_OK && c.n_words == (int32_t)words.size(), "code and count", k);
    if (c.rc != STR_ER_OK || c.n_words != (int32_t)words.size()) return;
    bool ok = true;
    for (size_t i = 0; i < words.size(); ++i) ok = ok && same_word(c.words[i], words[i]);
    for (size_t i = 0; i < word_of.size(); ++i) ok = ok && c.runs[i].word == word_of[i];
    int32_t at = 0;
    for (size_t t = 0; t < lines.size(); ++t) {
        int32_t n = 0;
        for (const str_er_line_word &W : words) n += W.line == (int32_t)t;
        ok = ok && c.lw[t].first_word == at && c.lw[t].n_words == n && c.lw[t].reserved == 0 && c.lw[t].colmax == lines[t].colmax;
        at += n;
    }
    expect(ok, "words, run words and line records", k);
}

} // namespace

int main()
{
    // hand-made: two words of two and one runs, an empty line, a line of one run
    const std::vector<Line> hand = {{9, {run(10, 20, 5, 14, 60), run(22, 30, 3, 9, 20), run(33, 40, 6, 20, 15)}}, {0, {}}, {2, {run(1, 2, 0, 2, 2)}}};
    {
        const Call c = call(hand, 1, 3);
        expect(c.rc == STR_ER_OK && c.n_words == 3, "hand-made: three words");
        if (c.n_words == 3) {
            expect(same_word(c.words[0], str_er_line_word{0, 0, 2, 10, 3, 20, 11, 80}), "hand-made: word 0");
            expect(same_word(c.words[1], str_er_line_word{0, 2, 1, 33, 6, 7, 14, 15}), "hand-made: word 1");
            expect(same_word(c.words[2], str_er_line_word{2, 3, 1, 1, 0, 1, 2, 2}), "hand-made: word 2");
            expect(c.runs[0].word == 0 && c.runs[1].word == 0 && c.runs[2].word == 1 && c.runs[3].word == 2, "hand-made: run words");
            expect(c.lw[0].first_word == 0 && c.lw[0].n_words == 2 && c.lw[1].first_word == 2 && c.lw[1].n_words == 0 && c.lw[2].first_word == 2 && c.lw[2].n_words == 1,
                   "hand-made: line records");
        }
        agree(hand, 1, 3, -2);
        expect(call({}, 1, 3).rc == STR_ER_OK && call({}, 1, 3).n_words == 0, "no line at all");
        const Call small = call(hand, 1, 3, 2);
        expect(small.rc == STR_ER_ECAPACITY && small.n_words == 3, "capacity too small: the count still set");
    }
    // the break rule at its edges: colmax 9, 3 g >= 9 and 3 g >= 18
    const auto pair = [](int32_t gap) { return std::vector<Line>{{9, {run(0, 4, 0, 9, 20), run(4 + gap, 6 + gap, 0, 1, 2)}}}; };
    expect(call(pair(3), 1, 3).n_words == 2 && call(pair(2), 1, 3).n_words == 1, "colmax 9 at 1 / 3");
    expect(call(pair(6), 2, 3).n_words == 2 && call(pair(5), 2, 3).n_words == 1, "colmax 9 at 2 / 3");
    const std::vector<Line> far = {{16384, {run(0, 1, 0, 16384, 16384), run(2, 3, 0, 1, 1), run(65534, 65535, 0, 1, 1)}}};
    expect(call(far, 1, 65535).n_words == 3 && call(far, 65535, 1).n_words == 1, "(1, 65535) and (65535, 1)");
    // what is refused
    expect(!str_er_host::word_gap_ok(0, 3) && !str_er_host::word_gap_ok(65536, 3) && !str_er_host::word_gap_ok(1, 0) && !str_er_host::word_gap_ok(1, 65536) &&
           str_er_host::word_gap_ok(1, 65535) && str_er_host::word_gap_ok(65535, 1) && str_er_host::word_gap_ok(1, 3), "the range of the gap");
    expect(call(hand, 0, 3).rc == STR_ER_EINVAL && call(hand, 1, 65536).rc == STR_ER_EINVAL && call(hand, 65536, 1).rc == STR_ER_EINVAL, "num / den out of range");
    {
        std::vector<Line> v = hand; v[0].runs[1].pixels = 0;
        expect(call(v, 1, 3).rc == STR_ER_EINVAL, "a run without a pixel");
        v = hand; v[0].runs[1].x0 = 20;
        expect(call(v, 1, 3).rc == STR_ER_EINVAL, "touching runs");
        v = hand; v[0].runs[1].x0 = 15;
        expect(call(v, 1, 3).rc == STR_ER_EINVAL, "overlapping runs");
        v = hand; std::swap(v[0].runs[0], v[0].runs[2]);
        expect(call(v, 1, 3).rc == STR_ER_EINVAL, "unordered runs");
        v = hand; v[0].runs[0].x1 = 10;
        expect(call(v, 1, 3).rc == STR_ER_EINVAL, "an empty column interval");
        v = hand; v[2].runs[0].y1 = 0;
        expect(call(v, 1, 3).rc == STR_ER_EINVAL, "an empty row interval");
        v = hand; v[0].colmax = 0;
        expect(call(v, 1, 3).rc == STR_ER_EINVAL, "runs and colmax 0");
        Call c = call(hand, 1, 3);
        int32_t n = 0;
        c.lw[2].first_run = 2;
        expect(str_er_words_from_runs(c.runs.data(), 4, c.lw.data(), 3, 1, 3, nullptr, 0, &n) == STR_ER_EINVAL, "lists not back to back");
        c.lw[2].first_run = 3;
        expect(str_er_words_from_runs(c.runs.data(), 3, c.lw.data(), 3, 1, 3, nullptr, 0, &n) == STR_ER_EINVAL, "fewer runs than listed");
        expect(str_er_words_from_runs(c.runs.data(), 4, c.lw.data(), 2, 1, 3, nullptr, 0, &n) == STR_ER_EINVAL, "more runs than listed");
        expect(str_er_words_from_runs(nullptr, 4, c.lw.data(), 3, 1, 3, nullptr, 0, &n) == STR_ER_EINVAL, "runs missing");
        expect(str_er_words_from_runs(c.runs.data(), 4, nullptr, 3, 1, 3, nullptr, 0, &n) == STR_ER_EINVAL, "line records missing");
        expect(str_er_words_from_runs(c.runs.data(), 4, c.lw.data(), 3, 1, 3, nullptr, 0, nullptr) == STR_ER_EINVAL, "count missing");
        expect(str_er_words_from_runs(c.runs.data(), -1, c.lw.data(), 3, 1, 3, nullptr, 0, &n) == STR_ER_EINVAL, "negative runs");
        expect(str_er_words_from_runs(c.runs.data(), 4, c.lw.data(), 3, 1, 3, c.words.data(), -1, &n) == STR_ER_EINVAL, "negative capacity");
        expect(str_er_words_from_runs(c.runs.data(), 4, c.lw.data(), 3, 1, 3, nullptr, 0, &n) == STR_ER_OK && n == 3, "and the tables as they were: accepted");
    }
    // random run lists, at the default gap, at both extremes and at random ones
    std::mt19937 rng(20261018u);
    const auto below = [&](uint32_t n) { return (int32_t)(rng() % n); };
    for (long k = 0; k < 2000; ++k) {
        std::vector<Line> lines((size_t)below(7));
        for (Line &L : lines) {
            const int32_t n = below(10);
            L.colmax = n ? 1u + (uint32_t)below(k % 5 == 0 ? 16384 : 40) : 0u;
            int32_t x = below(30000);
            for (int32_t i = 0; i < n; ++i) {
                const int32_t w = 1 + below(25), y0 = below(400), h = 1 + below((int32_t)L.colmax);
                L.runs.push_back(run(x, x + w, y0, y0 + h, 1u + (uint32_t)below(w * h > 0 ? (uint32_t)(w * h) : 1u)));
                x += w + 1 + below(3 * (int32_t)(L.colmax > 60 ? 60 : L.colmax));
            }
        }
        const int m = (int)(k % 4);
        agree(lines, m == 0 ? 1 : m == 1 ? 1 : m == 2 ? 65535 : 1 + below(65535), m == 0 ? 3 : m == 1 ? 65535 : m == 2 ? 1 : 1 + below(65535), k);
    }
    printf("%ld cases, %ld wrong\n", cases, bad);
    return bad ? 1 : 0;
}
