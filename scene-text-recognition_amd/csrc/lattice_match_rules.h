// lattice_match_rules.h -- INTERNAL: the rules of the lexicon match of a word over its piece lattice (the contract is at
// str_er_lattice_match in str_er.h): the band of lengths, the lattice of a word's runs, the edit distance of one entry over it, the full
// table of one entry with its backtrack, and one word against a lexicon.  HIP-free and header-only, on word_match_rules.h (keys, the
// fold, the lexicon's checks) and run_split_rules.h (the pieces' order, the free segmentation): the host entry point
// (api_lattice_match.cpp: str_er_lattice_match_words_host) and tests/cpp/lattice_match_rules_check.cpp use this same code;
// lattice_match_kernels.hip states the same rules for the device and is held against the numpy reference (tests/lattice_match_ref.py),
// which is written from the definition.
#pragma once
#include "run_split_rules.h"
#include "word_match_rules.h"

#include <string.h>

namespace str_er_lm {

namespace rs = str_er_rs;
namespace wm = str_er_wm;

constexpr int MAX_NODES = 32;          // N of a word that is tried
constexpr int MAX_EDGES = 80;          // edges of such a word: 8 runs of 4 atoms with 10 edges each
constexpr int SRC_BYTES = 32;          // source bytes of a word: one per character of the winning entry

struct Params { int32_t ins = 64, del = 64, band = 2, split = 8; };

inline bool params_ok(int32_t ins, int32_t del, int32_t band, int32_t split) { return wm::params_ok(ins, del, band) && split >= 0 && split <= 255; }

// an entry of `len` characters is tried on a word of R runs and N atoms
inline int  len_lo(int64_t R, int band) { return R - band > 1 ? (int)(R - band) : 1; }
inline int  len_hi(int64_t N, int band) { return N + band < wm::MAX_LEN ? (int)(N + band) : wm::MAX_LEN; }
inline bool in_band(int64_t R, int64_t N, int len, int band) { return N <= MAX_NODES && len >= len_lo(R, band) && len <= len_hi(N, band); }

// N of a word: the atoms of its runs
inline int64_t word_nodes(const str_er_run_split *splits, int32_t first_run, int32_t n_of)
{
    int64_t n = 0;
    for (int32_t r = first_run; r < first_run + n_of; ++r) n += splits[r].n_cuts + 1;
    return n;
}

// The lattice of a word with N <= 32: of the node n >= 1 its local index j, the node its run starts at and, for the edge from the local
// node i < j, the row and the part (run, piece; -1: the whole run).
struct Lattice {
    int            N = 0, R = 0;
    int            j[MAX_NODES + 1], off[MAX_NODES + 1];
    const uint8_t *row[MAX_NODES + 1][rs::MAX_ATOMS];
    str_er_split_part part[MAX_NODES + 1][rs::MAX_ATOMS];
};

inline void build(Lattice &L, const str_er_run_split *splits, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t first_run, int32_t n_of)
{
    L.N = 0; L.R = n_of;
    for (int32_t r = first_run; r < first_run + n_of; ++r) {
        const str_er_run_split &S = splits[r];
        const int A = S.n_cuts + 1, off = L.N;
        for (int j = 1; j <= A; ++j) {
            const int n = ++L.N;
            L.j[n] = j; L.off[n] = off;
            for (int i = 0; i < j; ++i) {
                const int k = rs::piece_index(A, i, j);
                L.row[n][i] = k < 0 ? run_costs + (size_t)r * wm::ALPHABET : piece_costs + ((size_t)S.first_piece + (size_t)k) * wm::ALPHABET;
                L.part[n][i] = str_er_split_part{r, k < 0 ? -1 : S.first_piece + k};
            }
        }
    }
}

inline int32_t read(const uint8_t *row, int a, bool fold)
{
    const int b = fold ? wm::fold_partner(a) : a;
    return row[a] < row[b] ? row[a] : row[b];
}

// D[n][j] from the cells before it, the candidates in the contract's order; D(f, j) reads a cell.  *move (optional) receives the first
// candidate that attains the minimum: 2 * i for SUB(i), 2 * i + 1 for DEL(i), -1 for INS.
template <class Cell>
inline int32_t cell(const Lattice &L, int n, int j, const uint8_t *e, const Params &p, bool fold, const Cell &D, int *move = nullptr)
{
    if (n == 0) {
        if (move) *move = -1;
        return j * p.ins;
    }
    int32_t best = INT32_MAX;
    int     mv = -1;
    for (int i = 0; i < L.j[n]; ++i) {
        const int     f = L.off[n] + i;
        const int32_t s = i > 0 ? p.split : 0;
        if (j >= 1) {
            const int32_t sub = D(f, j - 1) + read(L.row[n][i], e[j - 1], fold) + s;
            if (sub < best) { best = sub; mv = 2 * i; }
        }
        const int32_t del = D(f, j) + p.del + s;
        if (del < best) { best = del; mv = 2 * i + 1; }
    }
    if (j >= 1) {
        const int32_t ins = D(n, j - 1) + p.ins;
        if (ins < best) { best = ins; mv = -1; }
    }
    if (move) *move = mv;
    return best;
}

// D[N][len] of the entry e (labels 0 .. 64) over the lattice: two columns over the nodes
inline int32_t entry_cost(const Lattice &L, const uint8_t *e, int len, const Params &p, bool fold)
{
    int32_t col[2][MAX_NODES + 1];
    for (int j = 0; j <= len; ++j) {
        int32_t *cur = col[j & 1], *old = col[(j & 1) ^ 1];
        for (int n = 0; n <= L.N; ++n) cur[n] = cell(L, n, j, e, p, fold, [&](int f, int jj) { return jj == j ? cur[f] : old[f]; });
    }
    return col[len & 1][L.N];
}

// the whole table of one entry
struct Table { int32_t D[MAX_NODES + 1][wm::MAX_LEN + 1]; };
inline int32_t fill_table(const Lattice &L, const uint8_t *e, int len, const Params &p, bool fold, Table &T)
{
    for (int j = 0; j <= len; ++j)
        for (int n = 0; n <= L.N; ++n) T.D[n][j] = cell(L, n, j, e, p, fold, [&](int f, int jj) { return T.D[f][jj]; });
    return T.D[L.N][len];
}

// The backtrack from (N, len): at every cell the first candidate that attains it.  parts receives the edges taken in word order (at
// most N), src the SRC_BYTES source bytes padded with 0xFF; returns the number of parts.
inline int backtrack(const Lattice &L, const uint8_t *e, int len, const Params &p, bool fold, const Table &T, str_er_split_part *parts, uint8_t *src, int32_t *n_del,
                     int32_t *n_ins)
{
    str_er_split_part back[MAX_NODES];
    uint8_t           from[wm::MAX_LEN];          // of a character: the parts taken before it was met, from the end; bit 7: inserted
    int               np = 0;
    *n_del = *n_ins = 0;
    memset(src, 0xFF, SRC_BYTES);
    for (int n = L.N, j = len; n > 0 || j > 0;) {
        int mv = -1;
        cell(L, n, j, e, p, fold, [&](int f, int jj) { return T.D[f][jj]; }, &mv);
        if (mv < 0) {          // INS: the character j is inserted at the node n
            from[j - 1] = (uint8_t)(np | 0x80);
            ++*n_ins;
            --j;
            continue;
        }
        const int i = mv >> 1;
        back[np] = L.part[n][i];
        if (mv & 1) ++*n_del;
        else { from[j - 1] = (uint8_t)np; --j; }
        ++np;
        n = L.off[n] + i;
    }
    // a read character: its part in word order; an inserted one: the parts that end at or before its node, all but those met before it
    for (int t = 0; t < len; ++t) src[t] = from[t] & 0x80 ? (uint8_t)(0x80 | (np - (from[t] & 0x7F))) : (uint8_t)(np - 1 - from[t]);
    for (int t = 0; t < np; ++t) parts[t] = back[np - 1 - t];
    return np;
}

// the word's str_er_word_split cost: every run segmented on the minima of its rows (the fold leaves a row's minimum as it is)
inline int32_t free_cost(const str_er_run_split *splits, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t first_run, int32_t n_of, int32_t split)
{
    int32_t sum = 0;
    for (int32_t r = first_run; r < first_run + n_of; ++r) {
        const str_er_run_split &S = splits[r];
        const int A = S.n_cuts + 1;
        int32_t   m[rs::MAX_ATOMS + 1][rs::MAX_ATOMS + 1] = {};
        for (int i = 0; i < A; ++i)
            for (int j = i + 1; j <= A; ++j) {
                const int k = rs::piece_index(A, i, j);
                m[i][j] = rs::row_min(k < 0 ? run_costs + (size_t)r * wm::ALPHABET : piece_costs + ((size_t)S.first_piece + (size_t)k) * wm::ALPHABET);
            }
        int     from[rs::MAX_ATOMS], to[rs::MAX_ATOMS];
        int32_t cost = 0;
        rs::segment_run(m, A, split, from, to, &cost);
        sum += cost;
    }
    return sum;
}

// One word against the whole lexicon (entries as labels, offsets[n + 1]), on one thread: the record with first_part left 0, the
// SRC_BYTES source bytes and the parts of the winner (at most MAX_NODES).
inline str_er_lattice_match match_word(const str_er_run_split *splits, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t first_run, int32_t n_of,
                                       const uint8_t *labels, const int32_t *offsets, int32_t n, const Params &p, bool fold, uint8_t *src, str_er_split_part *parts)
{
    str_er_lattice_match r{-1, -1, -1, -1, 0, 0, 0, 0, 0, 0};
    memset(src, 0xFF, SRC_BYTES);
    r.free_cost = free_cost(splits, run_costs, piece_costs, first_run, n_of, p.split);
    const int64_t N = word_nodes(splits, first_run, n_of);
    if (N > MAX_NODES) return r;
    Lattice L;
    build(L, splits, run_costs, piece_costs, first_run, n_of);
    wm::Best2 b;
    for (int32_t e = 0; e < n; ++e) {
        const int len = offsets[e + 1] - offsets[e];
        if (!in_band(n_of, N, len, p.band)) continue;
        ++r.n_tried;
        b.add(wm::make_key(entry_cost(L, labels + offsets[e], len, p, fold), e));
    }
    const str_er_word_match m = wm::make_match(b, r.free_cost, r.n_tried);
    r.entry = m.entry; r.cost = m.cost; r.second_entry = m.second_entry; r.second_cost = m.second_cost;
    if (r.entry >= 0) {
        Table          T;
        const uint8_t *e = labels + offsets[r.entry];
        const int      len = offsets[r.entry + 1] - offsets[r.entry];
        fill_table(L, e, len, p, fold, T);
        r.n_parts = backtrack(L, e, len, p, fold, T, parts, src, &r.n_del, &r.n_ins);
    }
    return r;
}

} // namespace str_er_lm
