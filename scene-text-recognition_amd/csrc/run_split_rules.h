// run_split_rules.h -- INTERNAL: the rules of the splitting of touching glyphs (the contract is at str_er_run_split in str_er.h): the
// check of its parameters, the cut columns of a run from its column counts, the enumeration of the pieces of a cut run and the
// segmentation of a run from the minima of the cost rows of its pieces.  HIP-free and header-only: the host entry points
// (api_run_split.cpp: str_er_cuts_from_counts, str_er_split_words_host) and tests/cpp/run_split_rules_check.cpp use this same code;
// run_split_kernels.hip states the same rules for the device and is held against the numpy reference (tests/run_split_ref.py), which
// is written from the definition.
#pragma once
#include "../../include/str_er.h"

#include <stdint.h>

namespace str_er_rs {

constexpr int ALPHABET = 65;          // bytes of a cost row
constexpr int MAX_CUTS = 3;           // cuts of a run
constexpr int MAX_ATOMS = MAX_CUTS + 1;
constexpr int MAX_PIECES = MAX_ATOMS * (MAX_ATOMS + 1) / 2 - 1;       // 9
constexpr int MAX_W = 1024;           // RUN_SPLIT_MAX_W: a wider run is not split
constexpr int MAX_PARTS = 32;         // parts of a word that is matched or decoded

inline bool params_ok(int32_t num, int32_t den, int32_t split_cost)
{
    return num >= 1 && num <= 65535 && den >= 1 && den <= 65535 && split_cost >= 0 && split_cost <= 255;
}

// floor(H * num / den) in 64 bits; a column count is 32 bits, so a quotient past them is every count's upper bound all the same
inline uint32_t threshold(int32_t H, int32_t num, int32_t den)
{
    const int64_t q = (int64_t)H * num / den;
    return q > (int64_t)UINT32_MAX ? UINT32_MAX : (uint32_t)q;
}

// The kept cut columns (relative to the run, ascending) of a run of W columns and H rows with the column counts n: the valleys at or
// below thr = floor(H * num / den) that touch neither end, the 3 with the smallest (depth, column) where there are more.  Returns
// their number; the unused entries of cut are -1.
inline int cuts_from_counts(const uint32_t *n, int32_t W, int32_t H, int32_t num, int32_t den, int32_t cut[MAX_CUTS])
{
    for (int k = 0; k < MAX_CUTS; ++k) cut[k] = -1;
    if (W > MAX_W || W < 3) return 0;
    const uint32_t thr = threshold(H, num, den);
    uint64_t key[MAX_CUTS + 1];          // depth << 32 | column, ascending
    int      kept = 0;
    for (int32_t c = 0; c < W;) {
        if (n[c] > thr) { ++c; continue; }
        const int32_t a = c;
        uint32_t d = n[c];
        int32_t  cf = c, cl = c;
        for (; c < W && n[c] <= thr; ++c) {
            if (n[c] < d) { d = n[c]; cf = c; }
            if (n[c] == d) cl = c;
        }
        if (a == 0 || c == W) continue;          // (an interval at either end is no valley)
        int at = kept;
        key[at] = (uint64_t)d << 32 | (uint32_t)((cf + cl) / 2);
        for (; at > 0 && key[at] < key[at - 1]; --at) { const uint64_t t = key[at]; key[at] = key[at - 1]; key[at - 1] = t; }
        if (kept < MAX_CUTS) ++kept;
    }
    for (int k = 0; k < kept; ++k) cut[k] = (int32_t)(uint32_t)key[k];
    for (int i = 1; i < kept; ++i)
        for (int k = i; k > 0 && cut[k] < cut[k - 1]; --k) { const int32_t t = cut[k]; cut[k] = cut[k - 1]; cut[k - 1] = t; }
    return kept;
}

// pieces of a run with n_cuts cuts: every (i, j), i < j, over the nodes 0 .. A but (0, A), ordered by (i, j)
inline int n_pieces(int n_cuts) { return n_cuts > 0 ? (n_cuts + 1) * (n_cuts + 2) / 2 - 1 : 0; }
inline int piece_index(int A, int i, int j)          // -1: the run itself
{
    if (i == 0) return j == A ? -1 : j - 1;
    return (A - 1) + (i - 1) * A - (i - 1) * i / 2 + (j - i - 1);
}
inline void piece_nodes(int A, int k, int &i, int &j)
{
    for (i = 0; i < A; ++i)
        for (j = i + 1; j <= A; ++j)
            if (piece_index(A, i, j) == k) return;
    i = j = -1;
}

inline int row_min(const uint8_t *row)
{
    int m = row[0];
    for (int a = 1; a < ALPHABET; ++a) m = row[a] < m ? row[a] : m;
    return m;
}

// The segmentation of a run of A atoms: m[i][j] the minimum of the cost row of piece (i, j).  from / to receive the nodes of the parts
// in run order; returns their number, *cost the run's D[A].
inline int segment_run(const int32_t m[MAX_ATOMS + 1][MAX_ATOMS + 1], int A, int32_t split, int from[MAX_ATOMS], int to[MAX_ATOMS], int32_t *cost)
{
    int32_t D[MAX_ATOMS + 1];
    int     pred[MAX_ATOMS + 1];
    D[0] = 0; pred[0] = 0;
    for (int j = 1; j <= A; ++j) {
        D[j] = D[0] + m[0][j]; pred[j] = 0;
        for (int i = 1; i < j; ++i) {
            const int32_t v = D[i] + m[i][j] + split;
            if (v < D[j]) { D[j] = v; pred[j] = i; }
        }
    }
    int n = 0;
    for (int j = A; j > 0; j = pred[j]) ++n;
    int at = n;
    for (int j = A; j > 0; j = pred[j]) { --at; from[at] = pred[j]; to[at] = j; }
    *cost = D[A];
    return n;
}

// the splits of n_runs runs index pieces inside n_pieces rows, with the piece count their cuts give
inline bool splits_ok(const str_er_run_split *splits, int32_t n_runs, int32_t n_pieces_all)
{
    for (int32_t r = 0; r < n_runs; ++r) {
        const str_er_run_split &S = splits[r];
        if (S.n_cuts < 0 || S.n_cuts > MAX_CUTS || S.n_pieces != n_pieces(S.n_cuts)) return false;
        if (S.n_pieces > 0 && (S.first_piece < 0 || (int64_t)S.first_piece + S.n_pieces > n_pieces_all)) return false;
    }
    return true;
}

// One word: the runs first_run .. first_run + n_of of splits with their rows (run_costs, piece_costs: 65 bytes a row).  parts receives
// the split sequence (at most MAX_ATOMS a run) and, where part_costs is not null, part_costs the parts' rows back to back.
inline str_er_word_split split_word(const str_er_run_split *splits, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t first_run, int32_t n_of,
                                    int32_t split, str_er_split_part *parts, uint8_t *part_costs)
{
    str_er_word_split w{0, 0, 0, 0};
    for (int32_t r = first_run; r < first_run + n_of; ++r) {
        const str_er_run_split &S = splits[r];
        const int A = S.n_cuts + 1;
        int32_t   m[MAX_ATOMS + 1][MAX_ATOMS + 1] = {};
        for (int i = 0; i < A; ++i)
            for (int j = i + 1; j <= A; ++j) {
                const int k = piece_index(A, i, j);
                m[i][j] = row_min(k < 0 ? run_costs + (size_t)r * ALPHABET : piece_costs + ((size_t)S.first_piece + (size_t)k) * ALPHABET);
            }
        int     from[MAX_ATOMS], to[MAX_ATOMS];
        int32_t cost = 0;
        const int np = segment_run(m, A, split, from, to, &cost);
        for (int t = 0; t < np; ++t) {
            const int k = piece_index(A, from[t], to[t]);
            parts[w.n_parts] = str_er_split_part{r, k < 0 ? -1 : S.first_piece + k};
            if (part_costs) {
                const uint8_t *row = k < 0 ? run_costs + (size_t)r * ALPHABET : piece_costs + ((size_t)S.first_piece + (size_t)k) * ALPHABET;
                for (int a = 0; a < ALPHABET; ++a) part_costs[(size_t)w.n_parts * ALPHABET + a] = row[a];
            }
            ++w.n_parts;
        }
        w.cost += cost;
        w.read_cost += m[0][A];
    }
    return w;
}

} // namespace str_er_rs
