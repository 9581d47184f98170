// line_decode_rules.h -- INTERNAL: the rules of the line decoder (the contract is at str_er_line_decode in str_er.h): the checks of its
// arguments, the gap costs from the geometry, and the recurrence over a line's cost rows, its gap costs and the bigram table with its
// backtrack, built on the run step of word_decode_rules.h.  HIP-free and header-only: the host entry points (api_line_decode.cpp:
// str_er_line_gap_costs, str_er_decode_lines_host), the detect call (the gap costs of its lines) and
// tests/cpp/line_decode_rules_check.cpp use this same code; line_decode_kernels.hip states the same rules for the device and is held
// against the numpy reference (tests/line_decode_ref.py), which is written from the definition.
#pragma once
#include "word_decode_rules.h"

#include <vector>

namespace str_er_ld {

namespace wd = str_er_wd;

constexpr int      MAX_ROWS = 1024;            // rows of a line that is decoded
constexpr int      OFF = 255;                  // a gap move that is off
constexpr int      MAX_WEIGHT = 127;
constexpr int      PER_ROW = 3;                // labels (and sources) a row can emit: SUB, INS and the break in front of it
constexpr uint16_t SRC_INS = 0x8000, SRC_BREAK = 0x4000;
constexpr int      BREAK_LABEL = wd::E;

// the bound of the contract: the all-SUB path of 1024 rows, every gap at its dearest move that is on, stays below INF, so INF never wins
static_assert(2 * 255 + (255 + 255 + 254 + 255) * (MAX_ROWS - 1) + 255 == 1043202 && 1043202 < wd::INF, "a line of MAX_ROWS rows against INF");
// ... and whatever a value carries, INF included, a row adds at most a gap (255 + 254), a SUB (255 + 255) and an INS (255 + 255) to it:
// every value stays below 2^25 and the device's keys (value << 7 | state, word_decode_device.h) cannot wrap
static_assert((int64_t)wd::INF + (int64_t)(509 + 510 + 510) * MAX_ROWS + 255 < (1 << 25), "a line's values against the keys");

inline bool weight_ok(int32_t w) { return w >= 0 && w <= MAX_WEIGHT; }

// the windows (first_row[t], n_of[t]) lie inside n_rows rows, in ascending order, none over another
inline bool lines_in_rows(int64_t n_rows, const int32_t *first, const int32_t *n_of, int64_t n_lines)
{
    int64_t at = 0;
    for (int64_t t = 0; t < n_lines; ++t) {
        if (first[t] < at || n_of[t] < 0 || (int64_t)first[t] + n_of[t] > n_rows) return false;
        at = (int64_t)first[t] + n_of[t];
    }
    return true;
}

// no gap of a line (the pairs of its rows but the first) has both moves off
inline bool gaps_ok(const uint8_t *gaps, const int32_t *first, const int32_t *n_of, int64_t n_lines)
{
    for (int64_t t = 0; t < n_lines; ++t)
        for (int64_t r = (int64_t)first[t] + 1; r < (int64_t)first[t] + n_of[t]; ++r)
            if (gaps[2 * r] == OFF && gaps[2 * r + 1] == OFF) return false;
    return true;
}

// (J, K) of a gap of g columns in a line of colmax at the word gap num / den and the weight w
inline void gap_pair(int64_t g, uint32_t colmax, int32_t num, int32_t den, int32_t w, uint8_t out[2])
{
    const int64_t q = 8 * (g < 0 ? 0 : g) * (int64_t)den / ((int64_t)num * (int64_t)colmax), x = q < 16 ? q : 16;
    out[0] = (uint8_t)(w * x / 8); out[1] = (uint8_t)(w * (16 - x) / 8);
}

// the gap costs of every row (2 * n_rows bytes): false on a row outside the runs or a line of more than one run with colmax 0; the
// windows are checked before (lines_in_rows)
inline bool gap_costs(const str_er_line_run *runs, int64_t n_runs, const int32_t *row_run, int64_t n_rows, const int32_t *first, const int32_t *n_of, const uint32_t *colmax,
                      int64_t n_lines, int32_t num, int32_t den, int32_t w, uint8_t *gaps)
{
    for (int64_t r = 0; r < n_rows; ++r) { gaps[2 * r] = 0; gaps[2 * r + 1] = OFF; }
    const auto run_of = [&](int64_t r) { return row_run ? (int64_t)row_run[r] : r; };
    for (int64_t t = 0; t < n_lines; ++t)
        for (int64_t r = first[t]; r < (int64_t)first[t] + n_of[t]; ++r) {
            const int64_t q = run_of(r);
            if (q < 0 || q >= n_runs) return false;
            if (r == first[t] || run_of(r - 1) == q) continue;
            if (colmax[t] == 0) return false;
            gap_pair((int64_t)runs[q].x0 - (int64_t)runs[run_of(r - 1)].x1, colmax[t], num, den, w, gaps + 2 * r);
        }
    return true;
}

// One line: the n cost rows C (65 bytes each, back to back) and their gap pairs G (2 bytes each; the first is not read) under B with
// the moves INS and DEL (0: off).  chars / src receive 3 * n entries, padded with 0xFF / 0xFFFF, word_of_row n values.
inline str_er_line_decode decode_line(const uint8_t *C, const uint8_t *G, int n, const uint8_t *B, int32_t ins, int32_t del, uint8_t *chars, uint16_t *src,
                                      int32_t *word_of_row)
{
    str_er_line_decode r{};
    n = n < 0 ? 0 : n;
    for (int k = 0; k < PER_ROW * n; ++k) { chars[k] = 0xFF; src[k] = 0xFFFF; }
    for (int i = 0; i < n; ++i) word_of_row[i] = -1;
    if (n > MAX_ROWS) { r.cost = -1; return r; }
    std::vector<wd::Step> steps((size_t)n * wd::STATES);
    std::vector<int16_t>  brk((size_t)n, -1);          // per row: the state the break in front of it comes from, -1: a join
    int32_t V[wd::STATES];
    for (int a = 0; a < wd::ALPHABET; ++a) V[a] = wd::INF;
    V[wd::E] = 0;
    for (int i = 1; i <= n; ++i) {
        if (i >= 2) {
            const int32_t J = G[2 * (i - 1)], K = G[2 * (i - 1) + 1];
            int     from = 0;
            int32_t X = wd::end_cost(V, B, &from) + K;          // (the break ends a word as the end of the string does)
            for (int a = 0; a < wd::STATES; ++a) V[a] = J == OFF ? wd::INF : V[a] + J;
            if (K != OFF && X < V[wd::E]) { V[wd::E] = X; brk[(size_t)i - 1] = (int16_t)from; }
        }
        wd::run_step(V, C + (size_t)(i - 1) * wd::ALPHABET, B, ins, del, steps.data() + (size_t)(i - 1) * wd::STATES);
    }
    int state = 0;
    r.cost = wd::end_cost(V, B, &state);
    // the backtrack writes the string from its end, into the tail of the slice
    int at = PER_ROW * n;
    for (int i = n; i >= 1; --i) {
        const wd::Step *st = steps.data() + (size_t)(i - 1) * wd::STATES;
        if (st[state].ins) {
            chars[--at] = (uint8_t)state; src[at] = (uint16_t)((i - 1) | SRC_INS);
            ++r.n_ins;
            state = st[state].ins_pred;
        }
        if (st[state].del) ++r.n_del;
        else {
            chars[--at] = (uint8_t)state; src[at] = (uint16_t)(i - 1);
            word_of_row[i - 1] = r.n_breaks;          // (the breaks behind it: turned round below)
            ++r.n_sub;
            state = st[state].sub_pred;
        }
        if (state == wd::E && brk[(size_t)i - 1] >= 0) {
            chars[--at] = (uint8_t)BREAK_LABEL; src[at] = (uint16_t)((i - 1) | SRC_BREAK);
            ++r.n_breaks;
            state = brk[(size_t)i - 1];
        }
    }
    r.n_chars = PER_ROW * n - at;
    for (int k = 0; k < r.n_chars; ++k) { chars[k] = chars[at + k]; src[k] = src[at + k]; }          // (at >= 1 where n >= 1: downwards, in ascending order)
    for (int k = r.n_chars; k < PER_ROW * n; ++k) { chars[k] = 0xFF; src[k] = 0xFFFF; }
    for (int i = 0; i < n; ++i)
        if (word_of_row[i] >= 0) word_of_row[i] = r.n_breaks - word_of_row[i];
    return r;
}

} // namespace str_er_ld
