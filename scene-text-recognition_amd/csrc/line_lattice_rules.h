// line_lattice_rules.h -- INTERNAL: the rules of the joint decode of a text line over the piece lattices of its runs (the contract is at
// str_er_line_lattice_decode in str_er.h): the checks of its arguments, the node slots, and the recurrence over the atoms' ends of all
// runs of a line -- the node step of lattice_decode_rules.h inside a run, the gap step of line_decode_rules.h between two runs -- with
// its backtrack.  HIP-free and header-only, built on rs::piece_index, wd::end_cost and the constants of both parents: the host entry
// point (api_line_lattice.cpp: str_er_lattice_decode_lines_host) and tests/cpp/line_lattice_rules_check.cpp use this same code;
// line_lattice_kernels.hip states the same rules for the device and is held against the numpy reference (tests/line_lattice_ref.py),
// which is written from the definition.
#pragma once
#include "lattice_decode_rules.h"
#include "line_decode_rules.h"

#include <vector>

namespace str_er_ld {

constexpr int LL_MAX_RUNS = MAX_ROWS;                               // runs of a line that is decoded
constexpr int LL_MAX_NODES = LL_MAX_RUNS * rs::MAX_ATOMS;           // ... so a line has at most so many nodes
constexpr int LL_PER_NODE = PER_ROW;                                // labels (and sources) a node can emit

// the bounds of the contract: the whole-run all-SUB path is the line decoder's own at 1024 rows, so INF never wins
static_assert(LL_MAX_RUNS == 1024 && LL_MAX_NODES == 4096, "the limits of a line");
static_assert(2 * 255 + (255 + 255 + 254 + 255) * (LL_MAX_RUNS - 1) + 255 == 1043202 && 1043202 < wd::INF, "a line of LL_MAX_RUNS whole runs against INF");
// ... and whatever a value carries, INF included, a node adds at most a gap (255 + 254), a SUB (255 + 255), SPLIT (255) and an INS
// (255 + 255) to it: every value stays below 2^25 and the device's keys (value << 7 | state) cannot wrap
static_assert((int64_t)wd::INF + (int64_t)LL_MAX_NODES * (509 + 510 + 255 + 510) + 255 == 8356095 && 8356095 < (1 << 25), "a line's values against the keys");

// the node slot of every run: the atoms of the runs before it; slots[n_runs] their sum.  False above 2^31 - 1 (n_cuts checked before)
inline bool ll_node_slots(const str_er_run_split *splits, int64_t n_runs, std::vector<int32_t> &slots)
{
    slots.assign((size_t)n_runs + 1, 0);
    int64_t at = 0;
    for (int64_t r = 0; r < n_runs; ++r) {
        slots[(size_t)r] = (int32_t)at;
        at += splits[r].n_cuts + 1;
        if (at > 0x7FFFFFFF / LL_PER_NODE) return false;
    }
    slots[(size_t)n_runs] = (int32_t)at;
    return true;
}

// One line: the runs first_run .. first_run + n_of of splits with their rows (run_costs, piece_costs: 65 bytes a row) and their gap
// pairs (gaps: 2 bytes a run, the pair of the line's first run is not read) under B with the moves INS, DEL (0: off) and the penalty
// SPLIT.  With N the atoms of the line's runs: chars / src receive 3 * N entries, padded with 0xFF / 0xFFFF; parts and word_of_part N
// entries, the first n_parts in line order, the others {-1, -1} and -1; first_part is left 0.
inline str_er_line_lattice_decode decode_line_lattice(const str_er_run_split *splits, const uint8_t *run_costs, const uint8_t *piece_costs, const uint8_t *gaps,
                                                      int32_t first_run, int32_t n_of, const uint8_t *B, int32_t ins, int32_t del, int32_t split, uint8_t *chars,
                                                      uint16_t *src, str_er_split_part *parts, int32_t *word_of_part)
{
    constexpr int STATES = wd::STATES, ALPHABET = wd::ALPHABET, E = wd::E;
    constexpr int32_t INF = wd::INF;
    str_er_line_lattice_decode r{};
    n_of = n_of < 0 ? 0 : n_of;
    const int64_t N64 = word_nodes(splits, first_run, n_of);
    for (int64_t k = 0; k < LL_PER_NODE * N64; ++k) { chars[k] = 0xFF; src[k] = 0xFFFF; }
    for (int64_t k = 0; k < N64; ++k) { parts[k] = str_er_split_part{-1, -1}; word_of_part[k] = -1; }
    if (n_of > LL_MAX_RUNS) { r.cost = -1; return r; }
    const int N = (int)N64;
    std::vector<Step>    steps((size_t)N * STATES, Step{0, 0, 0, 0, 0});
    std::vector<int32_t> Vs(((size_t)N + 1) * STATES), node_run((size_t)N + 1), node_j((size_t)N + 1);
    std::vector<int16_t> brk((size_t)n_of, -1);          // per run: the state the break in front of it comes from, -1: a join
    int32_t U[STATES];
    for (int a = 0; a < ALPHABET; ++a) Vs[(size_t)a] = INF;
    Vs[E] = 0;
    int n = 0;
    for (int32_t q = 0; q < n_of; ++q) {
        const int32_t           run = first_run + q;
        const str_er_run_split &S = splits[run];
        const int A = S.n_cuts + 1, off = n;
        if (q > 0) {          // the gap step of the line decoder, on V at the run's local node 0: no edge crosses a run boundary
            int32_t      *V = Vs.data() + (size_t)off * STATES;
            const int32_t J = gaps[2 * (size_t)run], K = gaps[2 * (size_t)run + 1];
            int           from = 0;
            const int32_t X = wd::end_cost(V, B, &from) + K;
            for (int a = 0; a < STATES; ++a) V[a] = J == OFF ? INF : V[a] + J;
            if (K != OFF && X < V[E]) { V[E] = X; brk[(size_t)q] = (int16_t)from; }
        }
        for (int j = 1; j <= A; ++j) {          // the node step of the lattice decoder
            ++n;
            node_run[(size_t)n] = run; node_j[(size_t)n] = j;
            Step *st = steps.data() + (size_t)(n - 1) * STATES;
            for (int x = 0; x < STATES; ++x) U[x] = INF;
            for (int i = 0; i < j; ++i) {
                const int32_t *Vf = Vs.data() + (size_t)(off + i) * STATES;
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
            int32_t *Vn = Vs.data() + (size_t)n * STATES;
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
    r.cost = wd::end_cost(Vs.data() + (size_t)N * STATES, B, &state);
    // the backtrack writes the string, the parts and their words from their ends, into the tails of the slices; a source counts the
    // parts from the end and a word the breaks behind it until n_parts and n_breaks are known
    int at = LL_PER_NODE * N, np = 0;
    for (n = N; n >= 1;) {
        const Step *st = steps.data() + (size_t)(n - 1) * STATES;
        if (st[state].ins) {
            chars[--at] = (uint8_t)state; src[at] = (uint16_t)(np | SRC_INS);
            ++r.n_ins;
            state = st[state].ins_pred;
        }
        const int32_t           run = node_run[(size_t)n];
        const str_er_run_split &S = splits[run];
        const int A = S.n_cuts + 1, j = node_j[(size_t)n], i = st[state].i, k = rs::piece_index(A, i, j);
        parts[N - 1 - np] = str_er_split_part{run, k < 0 ? -1 : S.first_piece + k};
        if (st[state].del) ++r.n_del;
        else {
            chars[--at] = (uint8_t)state; src[at] = (uint16_t)np;
            word_of_part[N - 1 - np] = r.n_breaks;
            ++r.n_sub;
            state = st[state].pred;
        }
        ++np;
        if (i == 0 && state == E && brk[(size_t)(run - first_run)] >= 0) {          // local node 0 of a run reached at the boundary: the break in front of the part
            chars[--at] = (uint8_t)BREAK_LABEL; src[at] = (uint16_t)((np - 1) | SRC_BREAK);
            ++r.n_breaks;
            state = brk[(size_t)(run - first_run)];
        }
        n -= j - i;
    }
    r.n_chars = LL_PER_NODE * N - at;
    r.n_parts = np;
    for (int k = 0; k < r.n_chars; ++k) {          // (at >= 1 where N >= 1: downwards, in ascending order)
        const uint16_t v = src[at + k];
        chars[k] = chars[at + k];
        src[k] = (uint16_t)((np - 1 - (v & 0x3FFF)) | (v & (SRC_INS | SRC_BREAK)));
    }
    for (int k = r.n_chars; k < LL_PER_NODE * N; ++k) { chars[k] = 0xFF; src[k] = 0xFFFF; }
    for (int k = 0; k < np; ++k) {
        const int32_t v = word_of_part[N - np + k];
        parts[k] = parts[N - np + k];
        word_of_part[k] = v >= 0 ? r.n_breaks - v : -1;
    }
    for (int k = np; k < N; ++k) { parts[k] = str_er_split_part{-1, -1}; word_of_part[k] = -1; }
    return r;
}

// no gap of a line (the pairs of its runs but the first) has both moves off
inline bool ll_gaps_ok(const uint8_t *gaps, const int32_t *first, const int32_t *n_of, int64_t n_lines) { return gaps_ok(gaps, first, n_of, n_lines); }

} // namespace str_er_ld
