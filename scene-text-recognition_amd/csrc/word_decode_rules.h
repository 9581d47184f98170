// word_decode_rules.h -- INTERNAL: the rules of the open-vocabulary word decoder (the contract is at str_er_word_decode in str_er.h):
// the checks of its arguments, the recurrence over a word's cost rows and the bigram table with its backtrack, read_cost and the table
// builder.  HIP-free and header-only, cost() and thresholds() from word_match_rules.h: the host entry points (api_word_decode.cpp:
// str_er_bigram_from_probs, str_er_decode_words_host) and tests/cpp/word_decode_rules_check.cpp use this same code;
// word_decode_kernels.hip states the same rules for the device and is held against the numpy reference (tests/word_decode_ref.py),
// which is written from the definition.
#pragma once
#include "word_match_rules.h"

#include <string.h>

namespace str_er_wd {

constexpr int     ALPHABET = str_er_wm::ALPHABET;      // the characters of str_er_ocr_char
constexpr int     STATES = ALPHABET + 1;               // ... and the word boundary
constexpr int     E = ALPHABET;
constexpr int     TABLE = STATES * STATES;             // bytes of a bigram table
constexpr int     MAX_RUNS = 32;                       // runs of a word that is decoded
constexpr int     MAX_CHARS = 2 * MAX_RUNS;            // labels (and sources) of a word's string
constexpr int32_t INF = 1 << 20;

inline bool params_ok(int32_t ins, int32_t del) { return ins >= 0 && ins <= 255 && del >= 0 && del <= 255; }

// B from the probabilities of b after a (tp: 65 x 65), of b first (start: 65) and of a last (end: 65); start / end null: 0 there
inline void table_from_probs(const double *tp, const double *start, const double *end, uint8_t out[TABLE])
{
    double T[str_er_wm::N_THRESH];
    str_er_wm::thresholds(T);
    for (int a = 0; a < ALPHABET; ++a) {
        for (int b = 0; b < ALPHABET; ++b) out[a * STATES + b] = str_er_wm::cost(tp[a * ALPHABET + b], T);
        out[a * STATES + E] = end ? str_er_wm::cost(end[a], T) : 0;
        out[E * STATES + a] = start ? str_er_wm::cost(start[a], T) : 0;
    }
    out[E * STATES + E] = 0;
}

// the cost under B of the plain reading of m rows: the first arg min of every row, all SUB, with the boundary terms (any m)
inline int32_t read_cost(const uint8_t *C, int m, const uint8_t *B)
{
    int     prev = E;
    int32_t s = 0;
    for (int i = 0; i < m; ++i) {
        const uint8_t *row = C + (size_t)i * ALPHABET;
        int r = 0;
        for (int a = 1; a < ALPHABET; ++a) r = row[a] < row[r] ? a : r;
        s += B[prev * STATES + r] + row[r];
        prev = r;
    }
    return s + B[prev * STATES + E];
}

// what the recurrence records per (run, state): the SUB predecessor, whether DEL replaced it, whether INS replaced that, and the U-level
// state the inserted character follows
struct Step { uint8_t sub_pred, del, ins, ins_pred; };

// One run of the recurrence: V_{i-1} in V becomes V_i under the row's 65 bytes, and st[0 .. 65] records the moves (the line decoder,
// line_decode_rules.h, takes the same step between its gaps)
inline void run_step(int32_t V[STATES], const uint8_t *row, const uint8_t *B, int32_t ins, int32_t del, Step *st)
{
    int32_t U[STATES];
    for (int b = 0; b < ALPHABET; ++b) {
        int32_t best = V[0] + B[b];
        int     pred = 0;
        for (int a = 1; a < STATES; ++a) {
            const int32_t v = V[a] + B[a * STATES + b];
            if (v < best) { best = v; pred = a; }
        }
        U[b] = best + row[b];
        st[b] = Step{(uint8_t)pred, 0, 0, 0};
    }
    U[E] = INF;
    st[E] = Step{0, 0, 0, 0};
    if (del > 0)
        for (int a = 0; a < STATES; ++a)
            if (V[a] + del < U[a]) { U[a] = V[a] + del; st[a].del = 1; }
    for (int c = 0; c < STATES; ++c) V[c] = U[c];
    if (ins > 0)
        for (int c = 0; c < ALPHABET; ++c) {
            int32_t best = U[0] + B[c];
            int     pred = 0;
            for (int b = 1; b < ALPHABET; ++b) {
                const int32_t v = U[b] + B[b * STATES + c];
                if (v < best) { best = v; pred = b; }
            }
            if (best + ins < U[c]) { V[c] = best + ins; st[c].ins = 1; st[c].ins_pred = (uint8_t)pred; }
        }
}

// the end of a string: min over a of V[a] + B[a][E] with the smallest a, which is the state the backtrack starts from
inline int32_t end_cost(const int32_t V[STATES], const uint8_t *B, int *state)
{
    int32_t cost = V[0] + B[E];
    *state = 0;
    for (int a = 1; a < STATES; ++a)
        if (V[a] + B[a * STATES + E] < cost) { cost = V[a] + B[a * STATES + E]; *state = a; }
    return cost;
}

// One word: the m cost rows C (65 bytes each, back to back) under B with the moves INS and DEL (0: off).  chars / src receive 64 bytes
// each, padded with 0xFF.
inline str_er_word_decode decode_word(const uint8_t *C, int m, const uint8_t *B, int32_t ins, int32_t del, uint8_t *chars, uint8_t *src)
{
    str_er_word_decode r{};
    memset(chars, 0xFF, MAX_CHARS);
    memset(src, 0xFF, MAX_CHARS);
    r.read_cost = read_cost(C, m, B);
    if (m > MAX_RUNS) { r.cost = -1; return r; }
    static_assert(sizeof(Step) == 4, "step");
    Step    steps[MAX_RUNS][STATES];
    int32_t V[STATES];
    for (int a = 0; a < ALPHABET; ++a) V[a] = INF;
    V[E] = 0;
    for (int i = 1; i <= m; ++i) run_step(V, C + (size_t)(i - 1) * ALPHABET, B, ins, del, steps[i - 1]);
    int state = 0;
    r.cost = end_cost(V, B, &state);
    // the backtrack writes the string from its end
    uint8_t lab[MAX_CHARS], from[MAX_CHARS];
    int     at = MAX_CHARS;
    for (int i = m; i >= 1; --i) {
        const Step *st = steps[i - 1];
        if (st[state].ins) {
            lab[--at] = (uint8_t)state; from[at] = (uint8_t)((i - 1) | 0x80);
            ++r.n_ins;
            state = st[state].ins_pred;
        }
        if (st[state].del) ++r.n_del;
        else {
            lab[--at] = (uint8_t)state; from[at] = (uint8_t)(i - 1);
            ++r.n_sub;
            state = st[state].sub_pred;
        }
    }
    r.n_chars = MAX_CHARS - at;
    memcpy(chars, lab + at, (size_t)r.n_chars);
    memcpy(src, from + at, (size_t)r.n_chars);
    return r;
}

} // namespace str_er_wd
