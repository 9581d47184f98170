// word_match_kernels.hip -- the lexicon matcher on the device (gfx950): k_run_costs turns class probabilities into cost rows,
// k_word_match runs the weighted edit distance of every word's glyph runs against every lexicon entry in its band of lengths and keeps
// the two smallest (cost, index) keys per (word, chunk), k_word_match_final merges a word's chunks.  Integers only and no atomics: the
// output is the same bytes every time.  The rules are stated for the host in word_match_rules.h; the contract is at str_er_word_match
// in str_er.h.  What the track match shares with these kernels is in word_match_device.h.
#include <hip/hip_runtime.h>

#include "word_match_device.h"
#include "word_match_kernels.h"

namespace str_er {

namespace {

constexpr int      WM_THREADS = 256, WM_WAVES = WM_THREADS / 64;

// ---- k_run_costs ------------------------------------------------------------------------------------------------------------------
// T[c] = M[c % 8] * 2^-(c / 8): the exponent field of the eight doubles nearest to 2^(-j/8) lowered by c / 8 (exact: all normal)
__device__ __forceinline__ double wm_threshold(int c)
{
    constexpr uint64_t M[8] = {0x3FF0000000000000ull, 0x3FED5818DCFBA487ull, 0x3FEAE89F995AD3ADull, 0x3FE8ACE5422AA0DBull,
                               0x3FE6A09E667F3BCDull, 0x3FE4BFDAD5362A27ull, 0x3FE306FE0A31B715ull, 0x3FE172B83C7D517Bull};
    return __longlong_as_double((long long)(M[c & 7] - ((uint64_t)(c >> 3) << 52)));
}

// the smallest c with p >= T[c], else 255: comparisons of doubles only (word_match_rules.h: cost)
__device__ __forceinline__ int wm_cost(double p, const double *T)
{
    if (!(p >= T[254])) return 255;
    int lo = 0, hi = 254;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p >= T[mid]) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// one thread per (run, character), in one pass: the class of a character comes from a table the workgroup makes of the model's labels
__global__ void __launch_bounds__(256) k_run_costs(const double *__restrict__ prob, int n, int k, const int32_t *__restrict__ labels, int fold,
                                                   uint8_t *__restrict__ cost)
{
    __shared__ double  T[256];
    __shared__ int32_t cls[WM_ALPHABET];
    const int tid = (int)threadIdx.x;
    if (tid < 255) T[tid] = wm_threshold(tid);
    if (tid < WM_ALPHABET) {
        int j = 0;
        while (j < k && labels[j] != tid) ++j;       // (the first class with the label)
        cls[tid] = j < k ? j : -1;
    }
    __syncthreads();
    const size_t total = (size_t)n * WM_ALPHABET;
    for (size_t t = (size_t)blockIdx.x * 256 + tid; t < total; t += (size_t)gridDim.x * 256) {
        const size_t  r = t / WM_ALPHABET;
        const int     a = (int)(t - r * WM_ALPHABET);
        const double *p = prob + r * (size_t)k;
        const int     j = cls[a];
        int           c = j < 0 ? 255 : wm_cost(p[j], T);
        const int     b = wm_partner(a);
        if (fold && b != a) {
            const int jb = cls[b];
            const int cb = jb < 0 ? 255 : wm_cost(p[jb], T);
            c = cb < c ? cb : c;
        }
        cost[t] = (uint8_t)c;
    }
}

// ---- k_word_match -----------------------------------------------------------------------------------------------------------------
// The groups [g0, g1) of one chunk against the word whose cost rows are staged in ct: a wave takes every WM_WAVES-th group, a lane
// one entry; the two smallest keys of the lane.
template <int MC>
__device__ __forceinline__ void wm_chunk(const WmLexDev &lex, const uint8_t *ct, int g0, int g1, int len_lo, int m, int ins, int del, uint64_t &k1, uint64_t &k2)
{
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    for (int g = g0 + wave; g < g1; g += WM_WAVES) {
        const int gu = __builtin_amdgcn_readfirstlane(g);
        int       len = len_lo;
        while (gu >= lex.len_first[len + 1]) ++len;          // (gu < g1 <= len_first[len_hi + 1]: it ends inside the table)
        const int32_t idx = lex.index[(size_t)gu * WM_GROUP + lane];
        const int     c = wm_entry_cost<MC>(ct, lex.chars + lex.goff[gu] + lane, len, m, ins, del);
        if (idx >= 0) wm_add(k1, k2, (uint64_t)(uint32_t)c << 32 | (uint32_t)idx);
    }
}

// grid (chunks, words).  m is uniform per workgroup and the length per wave.
__global__ void __launch_bounds__(WM_THREADS) k_word_match(WmLexDev lex, WmParams prm, const uint8_t *__restrict__ costs, const int32_t *__restrict__ first_run,
                                                           const int32_t *__restrict__ n_of, uint64_t *__restrict__ partial)
{
    __shared__ uint8_t  ct[WM_ALPHABET * 32];
    __shared__ uint64_t wk[WM_WAVES][2];
    const int w = (int)blockIdx.y, chunk = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int m = n_of[w];
    uint64_t *out = partial + ((size_t)w * gridDim.x + chunk) * 2;
    const int len_lo = max(1, m - prm.band), len_hi = min(32, m + prm.band);
    int       g0 = 0, g1 = 0;
    if (m <= 32 && len_lo <= len_hi) {
        g0 = lex.len_first[len_lo] + chunk * WM_CHUNK_GROUPS;
        g1 = min(lex.len_first[len_hi + 1], g0 + WM_CHUNK_GROUPS);
    }
    if (g0 >= g1) {          // (uniform: nothing of this word in this chunk)
        if (tid == 0) { out[0] = WM_NO_KEY; out[1] = WM_NO_KEY; }
        return;
    }
    // the word's cost rows into LDS, folded where the lexicon folds case; rows past m cost 255 (they are never read out)
    const int      MC = m <= 8 ? 8 : m <= 16 ? 16 : 32;
    const uint8_t *C = costs + (size_t)first_run[w] * WM_ALPHABET;
    for (int t = tid; t < MC * WM_ALPHABET; t += WM_THREADS) {
        const int i = t / WM_ALPHABET, a = t - i * WM_ALPHABET;
        int       v = 255;
        if (i < m) {
            v = C[i * WM_ALPHABET + a];
            if (lex.fold) v = min(v, (int)C[i * WM_ALPHABET + wm_partner(a)]);
        }
        ct[t] = (uint8_t)v;
    }
    __syncthreads();
    uint64_t k1 = WM_NO_KEY, k2 = WM_NO_KEY;
    if (MC == 8) wm_chunk<8>(lex, ct, g0, g1, len_lo, m, prm.ins, prm.del, k1, k2);
    else if (MC == 16) wm_chunk<16>(lex, ct, g0, g1, len_lo, m, prm.ins, prm.del, k1, k2);
    else wm_chunk<32>(lex, ct, g0, g1, len_lo, m, prm.ins, prm.del, k1, k2);
    // the wave's two smallest by a butterfly (every lane ends with them), the workgroup's through LDS
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t o1 = wm_shfl_xor(k1, off), o2 = wm_shfl_xor(k2, off);
        const uint64_t lo = min(k1, o1), hi = max(k1, o1);
        k2 = min(hi, min(k2, o2));
        k1 = lo;
    }
    if ((tid & 63) == 0) { wk[tid >> 6][0] = k1; wk[tid >> 6][1] = k2; }
    __syncthreads();
    if (tid == 0) {
        uint64_t b1 = WM_NO_KEY, b2 = WM_NO_KEY;
        for (int v = 0; v < WM_WAVES; ++v) { wm_add(b1, b2, wk[v][0]); wm_add(b1, b2, wk[v][1]); }
        out[0] = b1; out[1] = b2;
    }
}

// one thread per word: the chunks' pairs merged (NO_KEY never displaces a key), the free cost and the number of entries tried
__global__ void __launch_bounds__(64) k_word_match_final(WmLexDev lex, WmParams prm, const uint8_t *__restrict__ costs, const int32_t *__restrict__ first_run,
                                                         const int32_t *__restrict__ n_of, int n_words, int n_chunks, const uint64_t *__restrict__ partial,
                                                         int32_t *__restrict__ matches)
{
    const int w = (int)(blockIdx.x * 64 + threadIdx.x);
    if (w >= n_words) return;
    const int m = n_of[w];
    uint64_t  b1 = WM_NO_KEY, b2 = WM_NO_KEY;
    for (int ch = 0; ch < n_chunks; ++ch) {
        const uint64_t *p = partial + ((size_t)w * n_chunks + ch) * 2;
        wm_add(b1, b2, p[0]);
        wm_add(b1, b2, p[1]);
    }
    const uint8_t *C = costs + (size_t)first_run[w] * WM_ALPHABET;
    int32_t        fc = 0;
    for (int i = 0; i < m; ++i) {
        int lo = 255;
        for (int a = 0; a < WM_ALPHABET; ++a) lo = min(lo, (int)C[(size_t)i * WM_ALPHABET + a]);
        fc += lo;
    }
    const int len_lo = max(1, m - prm.band), len_hi = min(32, m + prm.band);
    int32_t  *o = matches + (size_t)w * 6;
    o[0] = b1 == WM_NO_KEY ? -1 : (int32_t)(uint32_t)b1;
    o[1] = b1 == WM_NO_KEY ? -1 : (int32_t)(b1 >> 32);
    o[2] = b2 == WM_NO_KEY ? -1 : (int32_t)(uint32_t)b2;
    o[3] = b2 == WM_NO_KEY ? -1 : (int32_t)(b2 >> 32);
    o[4] = fc;
    o[5] = m <= 32 && len_lo <= len_hi ? lex.len_count[len_hi + 1] - lex.len_count[len_lo] : 0;
}

} // namespace

void launch_run_costs(hipStream_t s, const double *prob, int n, int k, const int32_t *labels, bool fold, uint8_t *cost)
{
    if (n <= 0) return;
    const size_t total = (size_t)n * WM_ALPHABET;
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(k_run_costs, dim3(blocks), dim3(256), 0, s, prob, n, k, labels, fold ? 1 : 0, cost);
}

int wm_chunks(const WmLexDev &lex)
{
    return std::max(1, (lex.n_groups + WM_CHUNK_GROUPS - 1) / WM_CHUNK_GROUPS);
}

void launch_word_match(hipStream_t s, const WmLexDev &lex, const WmParams &p, const uint8_t *costs, const int32_t *first_run, const int32_t *n_of, int n_words,
                       uint64_t *partial, void *matches)
{
    if (n_words <= 0) return;
    const int n_chunks = wm_chunks(lex);
    // (the words are the grid's y: at most 65535 a launch)
    for (int w0 = 0; w0 < n_words; w0 += 65535) {
        const int nw = std::min(65535, n_words - w0);
        hipLaunchKernelGGL(k_word_match, dim3((unsigned)n_chunks, (unsigned)nw), dim3(WM_THREADS), 0, s, lex, p, costs, first_run + w0, n_of + w0,
                           partial + (size_t)w0 * n_chunks * 2);
    }
    hipLaunchKernelGGL(k_word_match_final, dim3((unsigned)((n_words + 63) / 64)), dim3(64), 0, s, lex, p, costs, first_run, n_of, n_words, n_chunks, partial,
                       static_cast<int32_t *>(matches));
}

} // namespace str_er
