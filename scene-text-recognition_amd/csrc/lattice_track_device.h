// lattice_track_device.h -- INTERNAL, device code: what the kernels of the track match over the members' piece lattices
// (lattice_track_kernels.hip) and of the track pool in lattice mode (track_pool_kernels.hip) share -- where a word's structure lies in
// its row of k_lattice_track_table's table, and the lattice band of lengths of a member.  The rules are stated for the host in
// lattice_track_rules.h.
#pragma once
#include <hip/hip_runtime.h>

#include "lattice_track_kernels.h"
#include "lattice_match_device.h"

namespace str_er {

namespace {

constexpr int LT_N = 0, LT_S0 = 1, LT_S1 = 2, LT_D0 = 3, LT_EROW = LT_D0 + LM_MAX_NODES + 1;      // a word's ints in the table

// bit l - 1 set iff max(1, R - band) <= l <= min(32, N + band) and N <= 32 (lattice_track_rules.h: len_mask_of)
__device__ __forceinline__ uint32_t lt_len_mask(int R, int N, int band)
{
    const int lo = max(1, R - band), hi = min(32, N + band);
    if (N > LM_MAX_NODES || lo > hi) return 0u;
    const int n = hi - lo + 1;
    return (n >= 32 ? ~0u : (1u << n) - 1u) << (lo - 1);
}

// The structure of one word (its runs first .. first + n_runs of splits) into its row T of the table, by one thread: N (33: more than
// 32 nodes), the two structure words, D[n][0] and the row of every (node, span) slot.  k_lattice_track_table makes it for every word of
// a call; the lattice decode pool makes it for the cells of a read.
__device__ __forceinline__ void lt_table_row(int32_t *__restrict__ T, int del, int split, const str_er_run_split *__restrict__ splits, int first, int n_runs)
{
    const int m = max(n_runs, 0), mr = min(m, LM_MAX_RUNS);
    for (int k = 0; k < LM_SLOTS; ++k) T[LT_EROW + k] = -1;
    int      N = 0;
    uint32_t s0 = 0, s1 = 0;
    T[LT_D0] = 0;
    for (int t = 0; t < mr; ++t) {
        const int A = lm_atoms(splits, first + t), fp = splits[first + t].first_piece;
        if (N + A > LM_MAX_NODES) { N = LM_MAX_NODES + 1; break; }
        for (int jl = 1; jl <= A; ++jl) {
            const int      n = N + jl;
            int            dn = 0x7FFFFFFF;
            const uint32_t bits = (uint32_t)(jl - 1) << (2 * ((n - 1) & 15));
            if (n <= 16) s0 |= bits;
            else s1 |= bits;
            for (int d = 1; d <= jl; ++d) {
                const int i = jl - d, k = lm_piece_index(A, i, jl);
                T[LT_EROW + (n - 1) * 4 + d - 1] = k < 0 ? first + t : (fp + k) | LM_PIECE;
                dn = min(dn, T[LT_D0 + n - d] + del + (i > 0 ? split : 0));          // (this thread's own writes)
            }
            T[LT_D0 + n] = dn;
        }
        N += A;
    }
    if (m > mr) N = LM_MAX_NODES + 1;
    for (int n = N + 1; n <= LM_MAX_NODES; ++n) T[LT_D0 + n] = 0;      // (past N: jl = 1, computed and not used)
    T[LT_N] = N; T[LT_S0] = (int32_t)s0; T[LT_S1] = (int32_t)s1;
}

} // namespace

} // namespace str_er
