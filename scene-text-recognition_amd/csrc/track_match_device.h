// track_match_device.h -- INTERNAL, device code: what the kernels of the track match (track_match_kernels.hip) and of the track pool
// (track_pool_kernels.hip) share -- the band of lengths of a member, the wave reductions and the length of a group of the lexicon.
// The rules are stated for the host in track_read_rules.h.
#pragma once
#include <hip/hip_runtime.h>

#include "track_match_kernels.h"
#include "word_match_device.h"

namespace str_er {

namespace {

// bit l - 1 set iff |l - m| <= band for a length l in 1 .. 32 and m <= 32 (track_read_rules.h: len_mask_of)
__device__ __forceinline__ uint32_t tm_len_mask(int m, int band)
{
    const int lo = max(1, m - band), hi = min(32, m + band);
    if (m > 32 || lo > hi) return 0u;
    const int n = hi - lo + 1;
    return (n >= 32 ? ~0u : (1u << n) - 1u) << (lo - 1);
}

__device__ __forceinline__ uint32_t tm_wave_or(uint32_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v |= (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}

__device__ __forceinline__ uint32_t tm_wave_sum(uint32_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}

// every lane ends with the wave's two smallest keys
__device__ __forceinline__ void tm_wave_best2(uint64_t &k1, uint64_t &k2)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t o1 = wm_shfl_xor(k1, off), o2 = wm_shfl_xor(k2, off);
        const uint64_t lo = min(k1, o1), hi = max(k1, o1);
        k2 = min(hi, min(k2, o2));
        k1 = lo;
    }
}

// the length of the entries of group g (g < n_groups: it ends inside the table)
__device__ __forceinline__ int tm_group_len(const WmLexDev &lex, int g)
{
    int len = 1;
    while (g >= lex.len_first[len + 1]) ++len;
    return len;
}

} // namespace

} // namespace str_er
