// word_match_device.h -- INTERNAL, device code: what the kernels of the lexicon matcher (word_match_kernels.hip) and of the track match
// (track_match_kernels.hip) share -- the case partner of a label, the best / second merge of keys and the edit distance of one
// entry against cost rows in LDS.  The rules are stated for the host in word_match_rules.h.
#pragma once
#include <hip/hip_runtime.h>

#include "word_match_kernels.h"

namespace str_er {

namespace {

constexpr int      WM_ALPHABET = 65;
constexpr uint64_t WM_NO_KEY = ~0ull;

__device__ __forceinline__ int wm_partner(int a) { return a >= 10 && a < 36 ? a + 26 : a >= 36 && a < 62 ? a - 26 : a; }

__device__ __forceinline__ void wm_add(uint64_t &k1, uint64_t &k2, uint64_t k)
{
    const uint64_t lo = k < k1 ? k : k1, hi = k < k1 ? k1 : k;       // (selects: k1 and k2 stay in registers)
    k2 = hi < k2 ? hi : k2;
    k1 = lo;
}

__device__ __forceinline__ uint64_t wm_shfl_xor(uint64_t v, int off)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
    return (uint64_t)hi << 32 | lo;
}

// The edit distance of the word's m <= MC runs against the lane's entry of `len` labels.  The column D[0 .. MC][j] over the runs lives
// in registers: every index is a compile-time constant (rows past m are computed and not used; the result is taken at row m).
// Layout of the cost rows in LDS, run-major as the caller gives them: ct[(i - 1) * 65 + a] = C_i[a], one byte read per run and
// character step.  The character-major layout (ct[a * MC + i - 1]: one or two wide reads per character step, the bytes taken out of the
// words with shifts) was measured as well and was 15 % slower: the kernel is bound by its vector ALU work, which the shifts add to, and
// the byte reads go to the LDS unit beside it (profiles/word_match.md).
template <int MC>
__device__ __forceinline__ int wm_entry_cost(const uint8_t *ct, const uint32_t *__restrict__ words, int len, int m, int ins, int del)
{
    int col[MC + 1];
#pragma unroll
    for (int i = 0; i <= MC; ++i) col[i] = i * del;
    for (int q = 0; q * 4 < len; ++q) {
        const uint32_t w = words[q * WM_GROUP];
        for (int jj = 0; jj < 4 && q * 4 + jj < len; ++jj) {
            const int a = (int)(w >> (8 * jj) & 0xFFu);
            int diag = col[0];
            col[0] = (q * 4 + jj + 1) * ins;
#pragma unroll
            for (int i = 1; i <= MC; ++i) {
                const int c = ct[(i - 1) * WM_ALPHABET + a];
                const int sub = diag + c, up = col[i - 1] + del, left = col[i] + ins;
                diag = col[i];
                col[i] = min(sub, min(up, left));
            }
        }
    }
    int res = col[0];
#pragma unroll
    for (int i = 1; i <= MC; ++i) res = i == m ? col[i] : res;
    return res;
}

} // namespace

} // namespace str_er
