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

} // namespace

} // namespace str_er
