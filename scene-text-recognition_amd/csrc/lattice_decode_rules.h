// lattice_decode_rules.h -- INTERNAL: the rules of the joint decode of a word over its piece lattice and the bigram table (the contract is
// at str_er_lattice_decode in str_er.h): the check of its arguments, the recurrence over the nodes of the word's runs and its backtrack.
// HIP-free and header-only, read_cost and the constants from word_decode_rules.h, the pieces' order from run_split_rules.h: the host
// entry point (api_lattice_decode.cpp: str_er_lattice_decode_words_host) and tests/cpp/lattice_decode_rules_check.cpp use this same
// code; lattice_decode_kernels.hip states the same rules for the device and is held against the numpy reference
// (tests/lattice_decode_ref.py), which is written from the definition.
#pragma once
#include "run_split_rules.h"
#include "word_decode_rules.h"

namespace str_er_ld {

namespace rs = str_er_rs;
namespace wd = str_er_wd;

constexpr int MAX_NODES = 32;          // N of a word that is decoded
constexpr int MAX_CHARS = wd::MAX_CHARS;

inline bool params_ok(int32_t ins, int32_t del, int32_t split) { return wd::params_ok(ins, del) && split >= 0 && split <= 255; }

// N of a word: the atoms of its runs
inline int64_t word_nodes(const str_er_run_split *splits, int32_t first_run, int32_t n_of)
{
    int64_t n = 0;
    for (int32_t r = first_run; r < first_run + n_of; ++r) n += splits[r].n_cuts + 1;
    return n;
}

// what the recurrence records per (node, state): the U-level move (the local node i it came from, DEL or SUB with its predecessor),
// whether INS replaced it and the U-level state the inserted character follows
struct Step { uint8_t i, pred, del, ins, ins_pred; };

// One word: the runs first_run .. first_run + n_of of splits with their rows (run_costs, piece_costs: 65 bytes a row) under B with the
// moves INS, DEL (0: off) and the penalty SPLIT.  chars / src receive 64 bytes each, padded with 0xFF; parts the lattice parts in
// word order (at most MAX_NODES of them); first_part is left 0.
inline str_er_lattice_decode decode_word(const str_er_run_split *splits, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t first_run, int32_t n_of,
                                         const uint8_t *B, int32_t ins, int32_t del, int32_t split, uint8_t *chars, uint8_t *src, str_er_split_part *parts)
{
    constexpr int STATES = wd::STATES, ALPHABET = wd::ALPHABET, E = wd::E;
    constexpr int32_t INF = wd::INF;
    str_er_lattice_decode r{};
    memset(chars, 0xFF, MAX_CHARS);
    memset(src, 0xFF, MAX_CHARS);
    r.read_cost = wd::read_cost(run_costs + (size_t)first_run * ALPHABET, n_of, B);
    const int64_t N64 = word_nodes(splits, first_run, n_of);
    if (N64 > MAX_NODES) { r.cost = -1; return r; }
    const int N = (int)N64;
    Step    steps[MAX_NODES][STATES];
    int32_t V[MAX_NODES + 1][STATES], U[STATES];
    int32_t node_run[MAX_NODES + 1], node_j[MAX_NODES + 1];          // of the node n >= 1: its run and its local index
    memset(steps, 0, sizeof steps);
    for (int a = 0; a < ALPHABET; ++a) V[0][a] = INF;
    V[0][E] = 0;
    int n = 0;
    for (int32_t run = first_run; run < first_run + n_of; ++run) {
        const str_er_run_split &S = splits[run];
        const int A = S.n_cuts + 1, off = n;
        for (int j = 1; j <= A; ++j) {
            ++n;
            node_run[n] = run; node_j[n] = j;
            Step *st = steps[n - 1];
            for (int x = 0; x < STATES; ++x) U[x] = INF;
            for (int i = 0; i < j; ++i) {
                const int32_t *Vf = V[off + i];
                const int      k = rs::piece_index(A, i, j);
                const uint8_t *row = k < 0 ? run_costs + (size_t)run * ALPHABET : piece_costs + ((size_t)S.first_piece + (size_t)k) * ALPHABET;
                const int32_t  s = i > 0 ? split : 0;
                for (int b = 0; b < ALPHABET; ++b) {
                    int32_t best = Vf[0] + B[b];
                    int     pred = 0;
                    for (int a = 1; a < STATES; ++a) {
                        const int32_t v = Vf[a] + B[a * STATES + b];
                        if (v < best) { best = v; pred = a; }
                    }
                    const int32_t sub = best + row[b] + s;
                    if (sub < U[b]) { U[b] = sub; st[b].i = (uint8_t)i; st[b].pred = (uint8_t)pred; st[b].del = 0; }
                }
                if (del > 0)
                    for (int a = 0; a < STATES; ++a) {
                        const int32_t d = Vf[a] + del + s;
                        if (d < U[a]) { U[a] = d; st[a].i = (uint8_t)i; st[a].pred = 0; st[a].del = 1; }
                    }
            }
            int32_t *Vn = V[n];
            for (int c = 0; c < STATES; ++c) Vn[c] = U[c];
            if (ins > 0)
                for (int c = 0; c < ALPHABET; ++c) {
                    int32_t best = U[0] + B[c];
                    int     pred = 0;
                    for (int b = 1; b < ALPHABET; ++b) {
                        const int32_t v = U[b] + B[b * STATES + c];
                        if (v < best) { best = v; pred = b; }
                    }
                    if (best + ins < U[c]) { Vn[c] = best + ins; st[c].ins = 1; st[c].ins_pred = (uint8_t)pred; }
                }
        }
    }
    int state = 0;
    r.cost = V[N][0] + B[E];
    for (int a = 1; a < STATES; ++a)
        if (V[N][a] + B[a * STATES + E] < r.cost) { r.cost = V[N][a] + B[a * STATES + E]; state = a; }
    // the backtrack writes the string and the parts from their ends; a source counts the parts from the end until n_parts is known
    uint8_t           lab[MAX_CHARS], from[MAX_CHARS];
    str_er_split_part back[MAX_NODES];
    int               at = MAX_CHARS, np = 0;
    for (n = N; n >= 1;) {
        const Step *st = steps[n - 1];
        if (st[state].ins) {
            lab[--at] = (uint8_t)state; from[at] = (uint8_t)(np | 0x80);
            ++r.n_ins;
            state = st[state].ins_pred;
        }
        const str_er_run_split &S = splits[node_run[n]];
        const int A = S.n_cuts + 1, j = node_j[n], i = st[state].i, k = rs::piece_index(A, i, j);
        back[np] = str_er_split_part{node_run[n], k < 0 ? -1 : S.first_piece + k};
        if (st[state].del) ++r.n_del;
        else {
            lab[--at] = (uint8_t)state; from[at] = (uint8_t)np;
            ++r.n_sub;
            state = st[state].pred;
        }
        ++np;
        n -= j - i;
    }
    r.n_chars = MAX_CHARS - at;
    r.n_parts = np;
    for (int t = 0; t < r.n_chars; ++t) {
        chars[t] = lab[at + t];
        src[t] = (uint8_t)((np - 1 - (from[at + t] & 0x7F)) | (from[at + t] & 0x80));
    }
    for (int t = 0; t < np; ++t) parts[t] = back[np - 1 - t];
    return r;
}

} // namespace str_er_ld
