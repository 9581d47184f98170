// word_margin_rules.h -- INTERNAL: the rules of the word decoder's margins (the contract is at str_er_word_margin in str_er.h): the
// min-marginals of the recurrence of word_decode_rules.h -- for every run and every reading of it the cost of the cheapest whole path
// that reads the run that way -- by one backward pass over the table beside the forward one, and from them the margin of every row and
// of the word.  HIP-free and header-only: the host entry point (api_word_margin.cpp: str_er_word_margins_host) and
// tests/cpp/word_margin_rules_check.cpp use this same code; word_margin_kernels.hip states the same rules for the device and is held
// against the numpy reference (tests/word_margin_ref.py), which is written from the definition.
#pragma once
#include "word_decode_rules.h"

namespace str_er_wd {

constexpr int MARGINALS = STATES;          // per row: the 65 readings and, at 65, the row dropped

// One word: the m cost rows C under B with INS and DEL, and the string the decoder made of them (chars / src: its 64 + 64 bytes,
// n_chars of them used).  row_margin receives 32 values (-1 past m), row_read and row_alt 32 bytes each (0xFF past m), marginals
// (null: not wanted) 32 x 66 values (-1 past m and where no path exists).
inline str_er_word_margin margins_word(const uint8_t *C, int m, const uint8_t *B, int32_t ins, int32_t del, const uint8_t *chars, const uint8_t *src, int n_chars,
                                       int32_t *row_margin, uint8_t *row_read, uint8_t *row_alt, int32_t *marginals)
{
    str_er_word_margin r{-1, -1, -1, -1};
    for (int i = 0; i < MAX_RUNS; ++i) { row_margin[i] = -1; row_read[i] = row_alt[i] = 0xFF; }
    if (marginals)
        for (int i = 0; i < MAX_RUNS * MARGINALS; ++i) marginals[i] = -1;
    if (m < 1 || m > MAX_RUNS) return r;
    // the forward pass of decode_word, every V_{i-1} and S_i kept
    constexpr int32_t inf = INF;
    int32_t V[MAX_RUNS + 1][STATES], S[MAX_RUNS][ALPHABET], U[STATES];
    for (int a = 0; a < ALPHABET; ++a) V[0][a] = inf;
    V[0][E] = 0;
    for (int i = 1; i <= m; ++i) {
        const uint8_t *row = C + (size_t)(i - 1) * ALPHABET;
        const int32_t *P = V[i - 1];
        for (int b = 0; b < ALPHABET; ++b) {
            int32_t best = P[0] + B[b];
            for (int a = 1; a < STATES; ++a) best = P[a] + B[a * STATES + b] < best ? P[a] + B[a * STATES + b] : best;
            U[b] = S[i - 1][b] = best + row[b];
        }
        U[E] = inf;
        if (del > 0)
            for (int a = 0; a < STATES; ++a)
                if (P[a] + del < U[a]) U[a] = P[a] + del;
        for (int c = 0; c < STATES; ++c) V[i][c] = U[c];
        if (ins > 0)
            for (int c = 0; c < ALPHABET; ++c) {
                int32_t best = U[0] + B[c];
                for (int b = 1; b < ALPHABET; ++b) best = U[b] + B[b * STATES + c] < best ? U[b] + B[b * STATES + c] : best;
                if (best + ins < U[c]) V[i][c] = best + ins;
            }
    }
    int32_t cost = V[m][0] + B[E];
    for (int a = 1; a < STATES; ++a) cost = V[m][a] + B[a * STATES + E] < cost ? V[m][a] + B[a * STATES + E] : cost;
    // the reading of every row: the label of the character whose source is the row, or 65
    uint8_t x[MAX_RUNS];
    for (int i = 0; i < m; ++i) x[i] = (uint8_t)E;
    for (int k = 0; k < n_chars && k < MAX_CHARS; ++k)
        if (!(src[k] & 0x80) && src[k] < m) x[src[k]] = chars[k];
    // the backward pass, the marginals and the margin of every row on the way
    int32_t G[STATES], GU[STATES], N[STATES], M[MARGINALS];
    for (int a = 0; a < STATES; ++a) G[a] = B[a * STATES + E];
    for (int i = m; i >= 1; --i) {
        const uint8_t *row = C + (size_t)(i - 1) * ALPHABET;
        for (int a = 0; a < STATES; ++a) GU[a] = G[a];
        if (ins > 0)
            for (int b = 0; b < ALPHABET; ++b) {
                int32_t best = B[b * STATES] + G[0];
                for (int c = 1; c < ALPHABET; ++c) best = B[b * STATES + c] + G[c] < best ? B[b * STATES + c] + G[c] : best;
                if (best + ins < GU[b]) GU[b] = best + ins;
            }
        for (int b = 0; b < ALPHABET; ++b) M[b] = S[i - 1][b] + GU[b];
        M[E] = -1;
        if (del > 0) {
            int32_t best = V[i - 1][0] + del + GU[0];
            for (int a = 1; a < STATES; ++a) best = V[i - 1][a] + del + GU[a] < best ? V[i - 1][a] + del + GU[a] : best;
            M[E] = best;
        }
        for (int k = 0; k < MARGINALS; ++k)
            if (M[k] >= inf) M[k] = -1;          // (no path: INF never wins)
        int32_t best = -1;
        int     alt = -1;
        for (int k = 0; k < MARGINALS; ++k)
            if (k != x[i - 1] && M[k] >= 0 && (best < 0 || M[k] < best)) { best = M[k]; alt = k; }
        row_margin[i - 1] = best - cost; row_read[i - 1] = x[i - 1]; row_alt[i - 1] = (uint8_t)alt;
        if (marginals)
            for (int k = 0; k < MARGINALS; ++k) marginals[(i - 1) * MARGINALS + k] = M[k];
        for (int a = 0; a < STATES; ++a) {
            int32_t nb = B[a * STATES] + row[0] + GU[0];
            for (int b = 1; b < ALPHABET; ++b) nb = B[a * STATES + b] + row[b] + GU[b] < nb ? B[a * STATES + b] + row[b] + GU[b] : nb;
            if (del > 0 && del + GU[a] < nb) nb = del + GU[a];
            N[a] = nb;
        }
        for (int a = 0; a < STATES; ++a) G[a] = N[a];
    }
    for (int i = 0; i < m; ++i)
        if (r.margin < 0 || row_margin[i] < r.margin) { r.margin = row_margin[i]; r.row = i; r.read = row_read[i]; r.alt = row_alt[i]; }
    return r;
}

} // namespace str_er_wd
