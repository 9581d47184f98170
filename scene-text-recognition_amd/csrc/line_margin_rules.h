// line_margin_rules.h -- INTERNAL: the rules of the line decoder's margins (the contract is at str_er_line_margin in str_er.h): the
// min-marginals of the recurrence of line_decode_rules.h -- for every row and every reading of it, and for every gap and either move at
// it, the cost of the cheapest whole path that does just that -- by one backward pass over the same rows, gaps and table beside the
// forward one, and from them the margin of every row, of every gap and of the line.  HIP-free and header-only: the host entry point
// (api_line_margin.cpp: str_er_line_margins_host) and tests/cpp/line_margin_rules_check.cpp use this same code;
// line_margin_kernels.hip states the same rules for the device and is held against the numpy reference (tests/line_margin_ref.py),
// which is written from the definition.
#pragma once
#include "line_decode_rules.h"

namespace str_er_lm {

namespace wd = str_er_wd;
namespace ld = str_er_ld;

constexpr int     MARGINALS = wd::STATES + 2;          // per row: the 65 readings, at 65 the row dropped, at 66 the join and at 67 the break in front of it
constexpr int     JOIN = wd::STATES, BREAK = wd::STATES + 1;
constexpr uint8_t NONE8 = 0xFF;

// the bound of the contract (line_decode_rules.h): a marginal that exists is at most 1043202, below INF = 2^20, so a margin is too and
// the key margin << 10 | row of a line's smallest margin fits 31 bits
static_assert(1043202 < wd::INF && wd::INF == (1 << 20) && ld::MAX_ROWS == (1 << 10), "a margin against the key of a line");
static_assert(((int64_t)(wd::INF - 1) << 10 | (ld::MAX_ROWS - 1)) < (int64_t)0x7FFFFFFF, "the key of a line");
// a backward value is finite: at most a gap (255 + 254), a SUB (255 + 255) and an INS (255 + 255) a row; with a forward value below 2^25
// a sum of the two stays far below 2^31
static_assert((int64_t)(509 + 510 + 510) * ld::MAX_ROWS + 255 < (1 << 21), "a line's backward values");

inline str_er_line_margin no_margin() { return str_er_line_margin{-1, -1, -1, -1, -1, -1, -1, -1}; }

// One line: the n cost rows C and their gap pairs G under B with INS and DEL, as decode_line takes them, and the string it made of them
// (chars / src, n_chars of them used).  row_margin and gap_margin receive n values (-1 where there is none), row_read, row_alt and
// gap_move n bytes (0xFF where there is none), marginals (null: not wanted) n x 68 values (-1 where no path exists).
inline str_er_line_margin margins_line(const uint8_t *C, const uint8_t *G, int n, const uint8_t *B, int32_t ins, int32_t del, const uint8_t *chars, const uint16_t *src,
                                       int n_chars, int32_t *row_margin, uint8_t *row_read, uint8_t *row_alt, int32_t *gap_margin, uint8_t *gap_move, int32_t *marginals)
{
    str_er_line_margin r = no_margin();
    n = n < 0 ? 0 : n;
    for (int i = 0; i < n; ++i) { row_margin[i] = gap_margin[i] = -1; row_read[i] = row_alt[i] = gap_move[i] = NONE8; }
    if (marginals)
        for (size_t k = 0; k < (size_t)n * MARGINALS; ++k) marginals[k] = -1;
    if (n < 1 || n > ld::MAX_ROWS) return r;
    constexpr int32_t inf = wd::INF;
    // the forward pass of decode_line, V_{i-1}, X_i and S_i of every row kept
    std::vector<int32_t>  Vs((size_t)n * wd::STATES), Ss((size_t)n * wd::ALPHABET), Xs((size_t)n, inf);
    std::vector<wd::Step> step(wd::STATES);
    int32_t V[wd::STATES];
    for (int a = 0; a < wd::ALPHABET; ++a) V[a] = inf;
    V[wd::E] = 0;
    for (int i = 1; i <= n; ++i) {
        for (int a = 0; a < wd::STATES; ++a) Vs[(size_t)(i - 1) * wd::STATES + a] = V[a];
        if (i >= 2) {
            const int32_t J = G[2 * (i - 1)], K = G[2 * (i - 1) + 1];
            int     from = 0;
            int32_t X = wd::end_cost(V, B, &from) + K;
            for (int a = 0; a < wd::STATES; ++a) V[a] = J == ld::OFF ? inf : V[a] + J;
            if (K != ld::OFF) { Xs[(size_t)i - 1] = X; if (X < V[wd::E]) V[wd::E] = X; }
        }
        const uint8_t *row = C + (size_t)(i - 1) * wd::ALPHABET;
        for (int b = 0; b < wd::ALPHABET; ++b) {          // (the SUB value before DEL is compared)
            int32_t best = V[0] + B[b];
            for (int a = 1; a < wd::STATES; ++a) best = V[a] + B[a * wd::STATES + b] < best ? V[a] + B[a * wd::STATES + b] : best;
            Ss[(size_t)(i - 1) * wd::ALPHABET + b] = best + row[b];
        }
        wd::run_step(V, row, B, ins, del, step.data());
    }
    int state = 0;
    const int32_t cost = wd::end_cost(V, B, &state);
    // the reading of every row and the move of every gap, from the decoded string
    for (int i = 0; i < n; ++i) { row_read[i] = (uint8_t)wd::E; gap_move[i] = i == 0 ? NONE8 : (uint8_t)0; }
    for (int k = 0; k < n_chars && k < ld::PER_ROW * n; ++k) {
        const int at = src[k] & 0x3FFF;
        if (at >= n) continue;
        if (!(src[k] & (ld::SRC_INS | ld::SRC_BREAK))) row_read[at] = chars[k];
        else if (src[k] & ld::SRC_BREAK && !(src[k] & ld::SRC_INS) && at >= 1) gap_move[at] = 1;
    }
    // the backward pass, the marginals and the margins on the way
    int32_t Gb[wd::STATES], GU[wd::STATES], H[wd::STATES], M[MARGINALS];
    for (int a = 0; a < wd::STATES; ++a) Gb[a] = B[a * wd::STATES + wd::E];
    for (int i = n; i >= 1; --i) {
        const uint8_t *row = C + (size_t)(i - 1) * wd::ALPHABET;
        const int32_t *P = Vs.data() + (size_t)(i - 1) * wd::STATES, *S = Ss.data() + (size_t)(i - 1) * wd::ALPHABET;
        const int32_t  J = i >= 2 ? G[2 * (i - 1)] : 0, K = i >= 2 ? G[2 * (i - 1) + 1] : ld::OFF, X = Xs[(size_t)i - 1];
        for (int a = 0; a < wd::STATES; ++a) GU[a] = Gb[a];
        if (ins > 0)
            for (int b = 0; b < wd::ALPHABET; ++b) {
                int32_t best = B[b * wd::STATES] + Gb[0];
                for (int c = 1; c < wd::ALPHABET; ++c) best = B[b * wd::STATES + c] + Gb[c] < best ? B[b * wd::STATES + c] + Gb[c] : best;
                if (best + ins < GU[b]) GU[b] = best + ins;
            }
        for (int a = 0; a < wd::STATES; ++a) {
            int32_t h = B[a * wd::STATES] + row[0] + GU[0];
            for (int b = 1; b < wd::ALPHABET; ++b) h = B[a * wd::STATES + b] + row[b] + GU[b] < h ? B[a * wd::STATES + b] + row[b] + GU[b] : h;
            if (del > 0 && del + GU[a] < h) h = del + GU[a];
            H[a] = h;
        }
        for (int b = 0; b < wd::ALPHABET; ++b) M[b] = S[b] + GU[b];
        M[wd::E] = M[JOIN] = M[BREAK] = -1;
        if (del > 0) {          // the row dropped: from W_i, the state vector behind the gap step
            int32_t best = inf;
            for (int a = 0; a < wd::STATES; ++a) {
                int32_t w = i == 1 ? P[a] : J == ld::OFF ? inf : P[a] + J;
                if (a == wd::E && K != ld::OFF && X < w) w = X;
                best = w + del + GU[a] < best ? w + del + GU[a] : best;
            }
            M[wd::E] = best;
        }
        if (i >= 2 && J != ld::OFF) {
            int32_t best = P[0] + J + H[0];
            for (int a = 1; a < wd::STATES; ++a) best = P[a] + J + H[a] < best ? P[a] + J + H[a] : best;
            M[JOIN] = best;
        }
        if (i >= 2 && K != ld::OFF) M[BREAK] = X + H[wd::E];
        for (int k = 0; k < MARGINALS; ++k)
            if (M[k] >= inf) M[k] = -1;          // (no path: INF never wins)
        int32_t best = -1;
        int     alt = -1;
        for (int k = 0; k < wd::STATES; ++k)
            if (k != row_read[i - 1] && M[k] >= 0 && (best < 0 || M[k] < best)) { best = M[k]; alt = k; }
        row_margin[i - 1] = best - cost; row_alt[i - 1] = (uint8_t)alt;
        if (i >= 2) {
            const int32_t other = M[gap_move[i - 1] ? JOIN : BREAK];
            gap_margin[i - 1] = other >= 0 ? other - cost : -1;
        }
        if (marginals)
            for (int k = 0; k < MARGINALS; ++k) marginals[(size_t)(i - 1) * MARGINALS + k] = M[k];
        if (i >= 2)
            for (int a = 0; a < wd::STATES; ++a) {
                int32_t g = inf << 5;          // (stays only for a gap with both moves off, which gaps_ok refuses)
                if (J != ld::OFF) g = J + H[a];
                if (K != ld::OFF && B[a * wd::STATES + wd::E] + K + H[wd::E] < g) g = B[a * wd::STATES + wd::E] + K + H[wd::E];
                Gb[a] = g;
            }
    }
    for (int i = 0; i < n; ++i) {
        if (r.read_margin < 0 || row_margin[i] < r.read_margin) { r.read_margin = row_margin[i]; r.row = i; r.read = row_read[i]; r.alt = row_alt[i]; }
        if (gap_margin[i] >= 0 && (r.gap_margin < 0 || gap_margin[i] < r.gap_margin)) { r.gap_margin = gap_margin[i]; r.gap = i; r.gap_move = gap_move[i]; }
    }
    r.margin = r.gap_margin >= 0 && r.gap_margin < r.read_margin ? r.gap_margin : r.read_margin;
    return r;
}

} // namespace str_er_lm
