// track_match_kernels.hip -- the track match on the device (gfx950): k_track_match sums, per entry of the lexicon, the edit distances
// of all usable members of a word track and keeps the two smallest (cost, index) keys per (track, chunk); k_track_match_final merges a
// track's chunks and computes, for the winning entry, every member's own cost and the best member.  Integers only, no atomics and no
// scratch: the output is the same bytes every time.  The rules are stated for the host in track_read_rules.h; the contract is at
// str_er_word_link in str_er.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "track_match_device.h"

namespace str_er {

namespace {

constexpr int TM_THREADS = 256, TM_WAVES = TM_THREADS / 64;
constexpr int TM_SLOT = 32 * WM_ALPHABET;                  // bytes of the staged member: up to 32 rows
constexpr int TM_WAVE_GROUPS = TM_CHUNK_GROUPS / TM_WAVES; // groups of a chunk that one wave takes

// grid (chunks of the whole lexicon, tracks).  The workgroup walks the track's members one at a time: the member's rows into LDS (folded
// where the lexicon folds, the bucket 8 / 16 / 32 per member), then every wave adds the member's cost of its groups' entries into its
// lanes' accumulators acc[group of the wave][thread].  The member, its bucket and a group's length are uniform per wave.  Staging four
// members between two barriers was measured as well and was 11 % slower (profiles/track_read.md).
__global__ void __launch_bounds__(TM_THREADS) k_track_match(WmLexDev lex, WmParams prm, const uint8_t *__restrict__ costs, const int32_t *__restrict__ first_run,
                                                            const int32_t *__restrict__ n_of, const int32_t *__restrict__ track_first,
                                                            const int32_t *__restrict__ track_count, const int32_t *__restrict__ members, uint64_t *__restrict__ partial)
{
    __shared__ uint8_t  ct[TM_SLOT];
    __shared__ int32_t  acc[TM_WAVE_GROUPS][TM_THREADS];
    __shared__ uint8_t  glen[TM_CHUNK_GROUPS];
    __shared__ uint32_t wmask[TM_WAVES];
    __shared__ uint64_t wk[TM_WAVES][2];
    const int t = (int)blockIdx.y, chunk = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int first = track_first[t], count = track_count[t];
    const int g0 = chunk * TM_CHUNK_GROUPS, g1 = min(lex.n_groups, g0 + TM_CHUNK_GROUPS);
    uint64_t *out = partial + ((size_t)t * gridDim.x + chunk) * 2;
    // the lengths the track tries: the union of its usable members' bands
    uint32_t mk = 0;
    for (int j = tid; j < count; j += TM_THREADS) mk |= tm_len_mask(n_of[members[first + j]], prm.band);
    mk = tm_wave_or(mk);
    if (lane == 0) wmask[wave] = mk;
    if (tid < TM_CHUNK_GROUPS) glen[tid] = (uint8_t)(g0 + tid < g1 ? tm_group_len(lex, g0 + tid) : 0);
    __syncthreads();
    uint32_t mask = 0;
#pragma unroll
    for (int v = 0; v < TM_WAVES; ++v) mask |= wmask[v];
    uint32_t here = 0;          // ... and those of them this chunk holds
    for (int g = g0; g < g1; ++g) here |= 1u << (glen[g - g0] - 1);
    if (!(mask & here)) {          // (uniform: nothing of this track in this chunk)
        if (tid == 0) { out[0] = WM_NO_KEY; out[1] = WM_NO_KEY; }
        return;
    }
#pragma unroll
    for (int gi = 0; gi < TM_WAVE_GROUPS; ++gi) acc[gi][tid] = 0;
    for (int j = 0; j < count; ++j) {
        const int w = __builtin_amdgcn_readfirstlane(members[first + j]), m = __builtin_amdgcn_readfirstlane(n_of[w]);
        if (m > 32) continue;          // (uniform: an unusable member)
        const int      MC = m <= 8 ? 8 : m <= 16 ? 16 : 32;
        const uint8_t *C = costs + (size_t)first_run[w] * WM_ALPHABET;
        __syncthreads();          // (the rows of the member before are read)
        for (int e = tid; e < MC * WM_ALPHABET; e += TM_THREADS) {          // rows past m cost 255 (they are never read out)
            const int i = e / WM_ALPHABET, a = e - i * WM_ALPHABET;
            int       v = 255;
            if (i < m) {
                v = C[i * WM_ALPHABET + a];
                if (lex.fold) v = min(v, (int)C[i * WM_ALPHABET + wm_partner(a)]);
            }
            ct[e] = (uint8_t)v;
        }
        __syncthreads();
#pragma unroll 1
        for (int gi = 0; gi < TM_WAVE_GROUPS; ++gi) {
            const int gu = __builtin_amdgcn_readfirstlane(g0 + wave + gi * TM_WAVES);
            if (gu >= g1) break;
            const int len = __builtin_amdgcn_readfirstlane((int)glen[gu - g0]);
            if (!(mask >> (len - 1) & 1u)) continue;          // (a length outside the union of bands)
            const uint32_t *words = lex.chars + lex.goff[gu] + lane;
            int             c;
            if (MC == 8) c = wm_entry_cost<8>(ct, words, len, m, prm.ins, prm.del);
            else if (MC == 16) c = wm_entry_cost<16>(ct, words, len, m, prm.ins, prm.del);
            else c = wm_entry_cost<32>(ct, words, len, m, prm.ins, prm.del);
            acc[gi][tid] += c;
        }
    }
    uint64_t k1 = WM_NO_KEY, k2 = WM_NO_KEY;
#pragma unroll 1
    for (int gi = 0; gi < TM_WAVE_GROUPS; ++gi) {
        const int gu = __builtin_amdgcn_readfirstlane(g0 + wave + gi * TM_WAVES);
        if (gu >= g1) break;
        if (!(mask >> (glen[gu - g0] - 1) & 1u)) continue;
        const int32_t idx = lex.index[(size_t)gu * WM_GROUP + lane];
        if (idx >= 0) wm_add(k1, k2, (uint64_t)(uint32_t)acc[gi][tid] << 32 | (uint32_t)idx);
    }
    tm_wave_best2(k1, k2);
    if (lane == 0) { wk[wave][0] = k1; wk[wave][1] = k2; }
    __syncthreads();
    if (tid == 0) {
        uint64_t b1 = WM_NO_KEY, b2 = WM_NO_KEY;
        for (int v = 0; v < TM_WAVES; ++v) { wm_add(b1, b2, wk[v][0]); wm_add(b1, b2, wk[v][1]); }
        out[0] = b1; out[1] = b2;
    }
}

// D[m][len] of one member for the entry whose labels are at `words` (stride WM_GROUP), the member's rows read where they lie: one
// lane a member, so m differs between the lanes and the column takes the largest bucket; rows past m are not read.
__device__ __forceinline__ int tm_member_cost(const uint8_t *__restrict__ C, int m, int fold, const uint32_t *__restrict__ words, int len, int ins, int del)
{
    int col[33];
#pragma unroll
    for (int i = 0; i <= 32; ++i) col[i] = i * del;
    for (int j = 0; j < len; ++j) {
        const int a = (int)(words[(j >> 2) * WM_GROUP] >> (8 * (j & 3)) & 0xFFu), b = fold ? wm_partner(a) : a;
        int diag = col[0];
        col[0] = (j + 1) * ins;
#pragma unroll
        for (int i = 1; i <= 32; ++i) {
            int c = 255;
            if (i <= m) c = min((int)C[(i - 1) * WM_ALPHABET + a], (int)C[(i - 1) * WM_ALPHABET + b]);
            const int sub = diag + c, up = col[i - 1] + del, left = col[i] + ins;
            diag = col[i];
            col[i] = min(sub, min(up, left));
        }
    }
    int res = col[0];
#pragma unroll
    for (int i = 1; i <= 32; ++i) res = i == m ? col[i] : res;
    return res;
}

// one wave per track: the chunks' pairs merged, the free cost, the entries tried and the usable members counted, and for the winning
// entry every member's own cost and the best member.  A lane takes every 64th chunk and every 64th member.
__global__ void __launch_bounds__(64) k_track_match_final(WmLexDev lex, WmParams prm, const uint8_t *__restrict__ costs, const int32_t *__restrict__ first_run,
                                                          const int32_t *__restrict__ n_of, const int32_t *__restrict__ track_first,
                                                          const int32_t *__restrict__ track_count, const int32_t *__restrict__ members, int n_chunks,
                                                          const uint64_t *__restrict__ partial, int32_t *__restrict__ matches, int32_t *__restrict__ member_cost)
{
    const int t = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int first = track_first[t], count = track_count[t];
    uint64_t  k1 = WM_NO_KEY, k2 = WM_NO_KEY;
    for (int ch = lane; ch < n_chunks; ch += 64) {
        const uint64_t *p = partial + ((size_t)t * n_chunks + ch) * 2;
        wm_add(k1, k2, p[0]);
        wm_add(k1, k2, p[1]);
    }
    tm_wave_best2(k1, k2);
    uint32_t mk = 0, fc = 0, used = 0;
    for (int j = lane; j < count; j += 64) {
        const int      w = members[first + j], m = n_of[w];
        const uint8_t *C = costs + (size_t)first_run[w] * WM_ALPHABET;
        mk |= tm_len_mask(m, prm.band);
        used += m <= 32 ? 1u : 0u;
        for (int i = 0; i < m; ++i) {
            int lo = 255;
            for (int a = 0; a < WM_ALPHABET; ++a) lo = min(lo, (int)C[(size_t)i * WM_ALPHABET + a]);
            fc += (uint32_t)lo;
        }
    }
    mk = tm_wave_or(mk); fc = tm_wave_sum(fc); used = tm_wave_sum(used);
    int32_t tried = 0;
    for (int len = 1; len <= 32; ++len)
        if (mk >> (len - 1) & 1u) tried += lex.len_count[len + 1] - lex.len_count[len];
    const int32_t entry = k1 == WM_NO_KEY ? -1 : (int32_t)(uint32_t)k1;
    // the winner's labels by its slot in the sorted lexicon
    const uint32_t *words = lex.chars;
    int             len = 0;
    if (entry >= 0) {
        const int pos = lex.pos[entry], g = pos / WM_GROUP;
        len = tm_group_len(lex, g);
        words = lex.chars + lex.goff[g] + (pos - g * WM_GROUP);
    }
    uint64_t best = WM_NO_KEY;
    for (int j = lane; j < count; j += 64) {
        const int w = members[first + j], m = n_of[w];
        int32_t   c = -1;
        if (entry >= 0 && m <= 32) {
            c = tm_member_cost(costs + (size_t)first_run[w] * WM_ALPHABET, m, lex.fold, words, len, prm.ins, prm.del);
            best = min(best, (uint64_t)(uint32_t)c << 32 | (uint32_t)j);
        }
        member_cost[first + j] = c;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) best = min(best, wm_shfl_xor(best, off));
    if (lane == 0) {
        int32_t *o = matches + (size_t)t * 8;
        o[0] = entry;
        o[1] = k1 == WM_NO_KEY ? -1 : (int32_t)(k1 >> 32);
        o[2] = k2 == WM_NO_KEY ? -1 : (int32_t)(uint32_t)k2;
        o[3] = k2 == WM_NO_KEY ? -1 : (int32_t)(k2 >> 32);
        o[4] = (int32_t)fc;
        o[5] = tried;
        o[6] = (int32_t)used;
        o[7] = best == WM_NO_KEY ? -1 : members[first + (int)(uint32_t)best];
    }
}

} // namespace

int tm_chunks(const WmLexDev &lex)
{
    return std::max(1, (lex.n_groups + TM_CHUNK_GROUPS - 1) / TM_CHUNK_GROUPS);
}

void launch_track_match(hipStream_t s, const WmLexDev &lex, const WmParams &p, const uint8_t *costs, const int32_t *first_run, const int32_t *n_of,
                        const int32_t *track_first, const int32_t *track_count, const int32_t *members, int n_tracks, uint64_t *partial, void *matches,
                        int32_t *member_cost)
{
    if (n_tracks <= 0) return;
    const int n_chunks = tm_chunks(lex);
    // (the tracks are the grid's y: at most 65535 a launch)
    for (int t0 = 0; t0 < n_tracks; t0 += 65535) {
        const dim3 grid((unsigned)n_chunks, (unsigned)std::min(65535, n_tracks - t0));
        uint64_t  *part = partial + (size_t)t0 * n_chunks * 2;
        hipLaunchKernelGGL(k_track_match, grid, dim3(TM_THREADS), 0, s, lex, p, costs, first_run, n_of, track_first + t0, track_count + t0, members, part);
    }
    hipLaunchKernelGGL(k_track_match_final, dim3((unsigned)n_tracks), dim3(64), 0, s, lex, p, costs, first_run, n_of, track_first, track_count, members, n_chunks,
                       partial, static_cast<int32_t *>(matches), member_cost);
}

} // namespace str_er
