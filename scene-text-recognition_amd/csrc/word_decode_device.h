// word_decode_device.h -- INTERNAL: the device pieces the bigram decoders share (word_decode_kernels.hip: k_word_decode,
// lattice_decode_kernels.hip: k_lattice_decode, word_margin_kernels.hip: k_word_margin,
// lattice_margin_kernels.hip: k_lattice_margin, line_decode_kernels.hip: k_line_decode, line_margin_kernels.hip: k_line_margin): the
// layout of the table in LDS, the wave-level syncs, the min-plus product of a state vector with the table for the targets 0 .. 63 and its turned-round form for the target 64 and the end of the word, and a step of the
// plain reading.  A value travels with its state as a key (value << 7 | state); every value of either decoder is below 2^21, so a key
// is below 2^28 and the sum of a key and a table byte << 7 cannot wrap.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#ifndef WD_READLANE
#define WD_READLANE 0
#endif

namespace str_er {

namespace {

constexpr int      WD_ALPHABET = 65, WD_STATES = 66, WD_E = 65, WD_ROW = 68, WD_MAX_RUNS = 32;
constexpr uint32_t WD_INF = 1u << 20;
// a back pointer: bits 0 .. 6 the SUB predecessor, 7 DEL, 8 INS, 9 .. 15 the U-level state an inserted character follows
constexpr uint32_t WD_DEL = 1u << 7, WD_INS = 1u << 8;

// what one lane writes another lane of the same wave reads: the wave runs in lockstep and its LDS operations complete in order
__device__ __forceinline__ void wd_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// what the lanes of a wave leave in device memory for each other (the scratch tables of k_line_decode and k_line_margin): as
// wd_wave_sync, with the stores of the wave completed
__device__ __forceinline__ void wd_global_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ uint32_t wd_wave_min(uint32_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off, 64));
    return v;
}

// min over the predecessors a in [0, N) of key[a] + (B[a][lane] << 7); bcol = the table's bytes at the lane's column.  Fully unrolled:
// every offset is an immediate.
template <int N>
__device__ __forceinline__ uint32_t wd_product(const uint32_t *key, uint32_t key_lo, uint32_t key_hi, const uint8_t *bcol)
{
    uint32_t best = ~0u;
#if WD_READLANE
#pragma unroll
    for (int a = 0; a < (N < 64 ? N : 64); ++a)
        best = min(best, (uint32_t)__builtin_amdgcn_readlane((int)key_lo, a) + ((uint32_t)bcol[a * WD_ROW] << 7));
#pragma unroll
    for (int a = 64; a < N; ++a)
        best = min(best, (uint32_t)__builtin_amdgcn_readlane((int)key_hi, a - 64) + ((uint32_t)bcol[a * WD_ROW] << 7));
#else
#pragma unroll
    for (int a = 0; a < N; ++a) best = min(best, key[a] + ((uint32_t)bcol[a * WD_ROW] << 7));
#endif
    return best;
}

// the same for the target 64 (column `col` = 64) or the end of the word (col = 65), turned round: a lane a predecessor, the states 64
// and 65 in the lanes 0 .. n_hi - 1; every lane gets the minimum
__device__ __forceinline__ uint32_t wd_column(const uint8_t *Bs, int lane, int col, uint32_t key_lo, uint32_t key_hi, int n_hi)
{
    uint32_t t = key_lo + ((uint32_t)Bs[lane * WD_ROW + col] << 7);
    if (lane < n_hi) t = min(t, key_hi + ((uint32_t)Bs[(64 + lane) * WD_ROW + col] << 7));
    return wd_wave_min(t);
}

// a step of the plain reading: the first arg min of the row (c: the lane's byte, c64 the row's last), its cost and the bigram to it
__device__ __forceinline__ void wd_read_step(const uint8_t *Bs, int lane, uint32_t c, uint32_t c64, int &prev, int32_t &rc)
{
    uint32_t k = c << 7 | (uint32_t)lane;
    if (lane == 0) k = min(k, c64 << 7 | 64u);
    k = wd_wave_min(k);
    const int r = (int)(k & 127u);
    rc += (int32_t)Bs[prev * WD_ROW + r] + (int32_t)(k >> 7);
    prev = r;
}

} // namespace

} // namespace str_er
