// lattice_track_kernels.hip -- the track match over the members' piece lattices on the device (gfx950): k_lattice_track_table builds the
// lattice structure of every word once, k_lattice_track_match sums, per entry of the lexicon, the lattice edit distances of all usable
// members of a word track and keeps the two smallest (cost, index) keys per (track, chunk), k_lattice_track_merge merges a track's
// chunks, k_lattice_track_members runs the winner's table and backtrack for every member slot, and k_lattice_track_best sums the free
// costs and picks the best member.  Integers only, no atomics and no scratch: the output is the same bytes every time.  The rules are
// stated for the host in lattice_track_rules.h; the contract is at str_er_lattice_track_member in str_er.h.
//
// k_lattice_track_match is k_track_match's member loop (track_match_kernels.hip) with the cost of a member taken from lm_entry_cost, or
// from wm_entry_cost where the member has no cut (lattice_match_device.h, word_match_device.h).  k_lattice_match builds a word's
// structure with one thread of its workgroup; here a workgroup meets a word once per member and chunk, so the structure of every word
// (N, the two structure words, D[n][0] and the row of every (node, span) slot) is made once by k_lattice_track_table, a thread a word,
// and staging a member is a parallel gather through that table.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "lattice_track_device.h"

namespace str_er {

namespace {

constexpr int LT_THREADS = 256, LT_WAVES = LT_THREADS / 64;
constexpr int LT_WAVE_GROUPS = TM_CHUNK_GROUPS / LT_WAVES;      // groups of a chunk that one wave takes
constexpr int LT_SLOT_WAVES = 4;                                // member slots of a workgroup of k_lattice_track_members: a wave each
static_assert(LT_EROW + LM_SLOTS == LT_TAB_INTS, "the table's row");

__device__ __forceinline__ uint32_t lt_wave_or(uint32_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v |= (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}

__device__ __forceinline__ uint32_t lt_wave_sum(uint32_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}

// every lane ends with the wave's two smallest keys
__device__ __forceinline__ void lt_wave_best2(uint64_t &k1, uint64_t &k2)
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
__device__ __forceinline__ int lt_group_len(const WmLexDev &lex, int g)
{
    int len = 1;
    while (g >= lex.len_first[len + 1]) ++len;
    return len;
}

// a thread a word: the structure k_lattice_match makes per workgroup, into the word's row of the table.  N = 33: more than 32 nodes.
__global__ void __launch_bounds__(64) k_lattice_track_table(int del, int split, const str_er_run_split *__restrict__ splits, const int32_t *__restrict__ first_run,
                                                            const int32_t *__restrict__ n_of, int n_words, int32_t *__restrict__ tab)
{
    const int w = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (w >= n_words) return;
    lt_table_row(tab + (size_t)w * LT_TAB_INTS, del, split, splits, first_run[w], n_of[w]);
}

// grid (chunks of the whole lexicon, tracks).  The workgroup walks the track's members one at a time: the rows of the member's (node,
// span) slots into LDS through the table (folded where the lexicon folds; the rows of an uncut member back to back, as the matcher lays
// them out), then every wave adds the member's cost of its groups' entries into its lanes' accumulators acc[group of the wave][thread].
// The member, its bucket 8 / 16 / 32, whether it has a cut, its structure words and a group's length are uniform per wave: every branch
// on them is.
__global__ void __launch_bounds__(LT_THREADS) k_lattice_track_match(WmLexDev lex, WmParams prm, int split, const uint8_t *__restrict__ run_costs,
                                                                    const uint8_t *__restrict__ piece_costs, const int32_t *__restrict__ n_of,
                                                                    const int32_t *__restrict__ tab, const int32_t *__restrict__ track_first,
                                                                    const int32_t *__restrict__ track_count, const int32_t *__restrict__ members,
                                                                    uint64_t *__restrict__ partial)
{
    __shared__ uint8_t  ct[LM_SLOTS * WM_ALPHABET];
    __shared__ int32_t  acc[LT_WAVE_GROUPS][LT_THREADS];
    __shared__ int      d0[LM_MAX_NODES + 1];
    __shared__ uint8_t  glen[TM_CHUNK_GROUPS];
    __shared__ uint32_t wmask[LT_WAVES];
    __shared__ uint64_t wk[LT_WAVES][2];
    const int t = (int)blockIdx.y, chunk = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int first = track_first[t], count = track_count[t];
    const int g0 = chunk * TM_CHUNK_GROUPS, g1 = min(lex.n_groups, g0 + TM_CHUNK_GROUPS);
    uint64_t *out = partial + ((size_t)t * gridDim.x + chunk) * 2;
    // the lengths the track tries: the union of its usable members' lattice bands
    uint32_t mk = 0;
    for (int j = tid; j < count; j += LT_THREADS) {
        const int w = members[first + j];
        mk |= lt_len_mask(max(n_of[w], 0), tab[(size_t)w * LT_TAB_INTS + LT_N], prm.band);
    }
    mk = lt_wave_or(mk);
    if (lane == 0) wmask[wave] = mk;
    if (tid < TM_CHUNK_GROUPS) glen[tid] = (uint8_t)(g0 + tid < g1 ? lt_group_len(lex, g0 + tid) : 0);
    __syncthreads();
    uint32_t mask = 0;
#pragma unroll
    for (int v = 0; v < LT_WAVES; ++v) mask |= wmask[v];
    uint32_t here = 0;          // ... and those of them this chunk holds
    for (int g = g0; g < g1; ++g) here |= 1u << (glen[g - g0] - 1);
    if (!(mask & here)) {          // (uniform: nothing of this track in this chunk)
        if (tid == 0) { out[0] = WM_NO_KEY; out[1] = WM_NO_KEY; }
        return;
    }
#pragma unroll
    for (int gi = 0; gi < LT_WAVE_GROUPS; ++gi) acc[gi][tid] = 0;
    for (int j = 0; j < count; ++j) {
        const int      w = __builtin_amdgcn_readfirstlane(members[first + j]);
        const int32_t *T = tab + (size_t)w * LT_TAB_INTS;
        const int      N = __builtin_amdgcn_readfirstlane(T[LT_N]);
        if (N > LM_MAX_NODES) continue;          // (uniform: an unusable member)
        const uint32_t S0 = (uint32_t)__builtin_amdgcn_readfirstlane(T[LT_S0]), S1 = (uint32_t)__builtin_amdgcn_readfirstlane(T[LT_S1]);
        const bool     cut = (S0 | S1) != 0;
        const int      MC = N <= 8 ? 8 : N <= 16 ? 16 : 32;
        __syncthreads();          // (the rows of the member before are read)
        if (tid <= LM_MAX_NODES) d0[tid] = T[LT_D0 + tid];
        for (int e = tid; e < (cut ? MC * 4 : MC) * WM_ALPHABET; e += LT_THREADS) {          // a slot without an edge costs 255 (it is never read out)
            const int     k = e / WM_ALPHABET, a = e - k * WM_ALPHABET;
            const int32_t at = T[LT_EROW + (cut ? k : 4 * k)];
            int           v = 255;
            if (at >= 0) {
                const uint8_t *C = at & LM_PIECE ? piece_costs + (size_t)(at & (LM_PIECE - 1)) * WM_ALPHABET : run_costs + (size_t)at * WM_ALPHABET;
                v = C[a];
                if (lex.fold) v = min(v, (int)C[wm_partner(a)]);
            }
            ct[e] = (uint8_t)v;
        }
        __syncthreads();
#pragma unroll 1
        for (int gi = 0; gi < LT_WAVE_GROUPS; ++gi) {
            const int gu = __builtin_amdgcn_readfirstlane(g0 + wave + gi * LT_WAVES);
            if (gu >= g1) break;
            const int len = __builtin_amdgcn_readfirstlane((int)glen[gu - g0]);
            if (!(mask >> (len - 1) & 1u)) continue;          // (a length outside the union of bands)
            const uint32_t *words = lex.chars + lex.goff[gu] + lane;
            int             c;
            if (cut) {
                if (MC == 8) c = lm_entry_cost<8>(ct, S0, S1, d0, words, len, N, prm.ins, prm.del, split);
                else if (MC == 16) c = lm_entry_cost<16>(ct, S0, S1, d0, words, len, N, prm.ins, prm.del, split);
                else c = lm_entry_cost<32>(ct, S0, S1, d0, words, len, N, prm.ins, prm.del, split);
            } else {
                if (MC == 8) c = wm_entry_cost<8>(ct, words, len, N, prm.ins, prm.del);
                else if (MC == 16) c = wm_entry_cost<16>(ct, words, len, N, prm.ins, prm.del);
                else c = wm_entry_cost<32>(ct, words, len, N, prm.ins, prm.del);
            }
            acc[gi][tid] += c;
        }
    }
    uint64_t k1 = WM_NO_KEY, k2 = WM_NO_KEY;
#pragma unroll 1
    for (int gi = 0; gi < LT_WAVE_GROUPS; ++gi) {
        const int gu = __builtin_amdgcn_readfirstlane(g0 + wave + gi * LT_WAVES);
        if (gu >= g1) break;
        if (!(mask >> (glen[gu - g0] - 1) & 1u)) continue;
        const int32_t idx = lex.index[(size_t)gu * WM_GROUP + lane];
        if (idx >= 0) wm_add(k1, k2, (uint64_t)(uint32_t)acc[gi][tid] << 32 | (uint32_t)idx);
    }
    lt_wave_best2(k1, k2);
    if (lane == 0) { wk[wave][0] = k1; wk[wave][1] = k2; }
    __syncthreads();
    if (tid == 0) {
        uint64_t b1 = WM_NO_KEY, b2 = WM_NO_KEY;
        for (int v = 0; v < LT_WAVES; ++v) { wm_add(b1, b2, wk[v][0]); wm_add(b1, b2, wk[v][1]); }
        out[0] = b1; out[1] = b2;
    }
}

// one wave per track: the chunks' pairs merged, the entries tried and the usable members counted.  A lane takes every 64th chunk and
// every 64th member.  free_cost and best_member are k_lattice_track_best's.
__global__ void __launch_bounds__(64) k_lattice_track_merge(WmLexDev lex, WmParams prm, const int32_t *__restrict__ n_of, const int32_t *__restrict__ tab,
                                                            const int32_t *__restrict__ track_first, const int32_t *__restrict__ track_count,
                                                            const int32_t *__restrict__ members, int n_chunks, const uint64_t *__restrict__ partial,
                                                            int32_t *__restrict__ matches)
{
    const int t = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int first = track_first[t], count = track_count[t];
    uint64_t  k1 = WM_NO_KEY, k2 = WM_NO_KEY;
    for (int ch = lane; ch < n_chunks; ch += 64) {
        const uint64_t *p = partial + ((size_t)t * n_chunks + ch) * 2;
        wm_add(k1, k2, p[0]);
        wm_add(k1, k2, p[1]);
    }
    lt_wave_best2(k1, k2);
    uint32_t mk = 0, used = 0;
    for (int j = lane; j < count; j += 64) {
        const int w = members[first + j], N = tab[(size_t)w * LT_TAB_INTS + LT_N];
        mk |= lt_len_mask(max(n_of[w], 0), N, prm.band);
        used += N <= LM_MAX_NODES ? 1u : 0u;
    }
    mk = lt_wave_or(mk); used = lt_wave_sum(used);
    int32_t tried = 0;
    for (int len = 1; len <= 32; ++len)
        if (mk >> (len - 1) & 1u) tried += lex.len_count[len + 1] - lex.len_count[len];
    if (lane == 0) {
        int32_t *o = matches + (size_t)t * 8;
        o[0] = k1 == WM_NO_KEY ? -1 : (int32_t)(uint32_t)k1;
        o[1] = k1 == WM_NO_KEY ? -1 : (int32_t)(k1 >> 32);
        o[2] = k2 == WM_NO_KEY ? -1 : (int32_t)(uint32_t)k2;
        o[3] = k2 == WM_NO_KEY ? -1 : (int32_t)(k2 >> 32);
        o[4] = 0;
        o[5] = tried;
        o[6] = (int32_t)used;
        o[7] = -1;
    }
}

// a wave per slot of the member array: the member's free cost, and for the entry of the slot's track its own table and backtrack
__global__ void __launch_bounds__(64 * LT_SLOT_WAVES) k_lattice_track_members(WmLexDev lex, WmParams prm, int split, const str_er_run_split *__restrict__ splits,
                                                                              const uint8_t *__restrict__ run_costs, const uint8_t *__restrict__ piece_costs,
                                                                              const int32_t *__restrict__ first_run, const int32_t *__restrict__ n_of,
                                                                              const int32_t *__restrict__ members, const int32_t *__restrict__ slot_track,
                                                                              const int32_t *__restrict__ pslot, int n_members, const int32_t *__restrict__ matches,
                                                                              int32_t *__restrict__ mrec, uint8_t *__restrict__ src, int32_t *__restrict__ parts,
                                                                              int32_t *__restrict__ mfree)
{
    __shared__ LmWaveLds lds[LT_SLOT_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sl = (int)blockIdx.x * LT_SLOT_WAVES + wave;
    if (sl >= n_members) return;          // (no workgroup barrier below: a wave is on its own)
    const int t = __builtin_amdgcn_readfirstlane(slot_track[sl]);
    int32_t  *o = mrec + (size_t)sl * 6;
    if (t < 0) {          // (uniform) a slot of no track
        if (lane < 32) src[(size_t)sl * 32 + lane] = 0xFF;
        if (lane == 0) { o[0] = -1; o[1] = o[2] = o[3] = o[4] = 0; o[5] = -1; mfree[sl] = 0; }
        return;
    }
    const int    w = __builtin_amdgcn_readfirstlane(members[sl]);
    const int    first = __builtin_amdgcn_readfirstlane(first_run[w]), m = max(0, __builtin_amdgcn_readfirstlane(n_of[w]));
    const size_t base = (size_t)__builtin_amdgcn_readfirstlane(pslot[sl]);
    const int    entry = __builtin_amdgcn_readfirstlane(matches[(size_t)t * 8]);
    LmWaveLds   &L = lds[wave];
    int          N = 0;
    const int32_t fc = lm_wave_nodes(L, splits, run_costs, piece_costs, first, m, split, lane, N);
    const bool    run = entry >= 0 && N <= LM_MAX_NODES;
    const int     len = lm_wave_winner(L, lex, prm, split, run_costs, piece_costs, entry, N, run, lane);
    lm_wave_sync();
    lm_wave_store(L, len, lane, src + (size_t)sl * 32, parts + 2 * base);          // (n_parts <= N: inside the slot's part slots)
    if (lane == 0) {
        o[0] = run ? L.T[N * LM_TROW + len] : -1;
        o[1] = 0; o[2] = L.rec[0]; o[3] = L.rec[1]; o[4] = L.rec[2]; o[5] = w;
        mfree[sl] = fc;
    }
}

// one wave per track: the sum of the members' free costs and the member with the smallest cost, ties to the earliest slot
__global__ void __launch_bounds__(64) k_lattice_track_best(const int32_t *__restrict__ track_first, const int32_t *__restrict__ track_count,
                                                           const int32_t *__restrict__ members, const int32_t *__restrict__ mrec, const int32_t *__restrict__ mfree,
                                                           int32_t *__restrict__ matches)
{
    const int t = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int first = track_first[t], count = track_count[t];
    uint32_t  fc = 0;
    uint64_t  best = WM_NO_KEY;
    for (int j = lane; j < count; j += 64) {
        const int32_t c = mrec[(size_t)(first + j) * 6];
        fc += (uint32_t)mfree[first + j];
        if (c >= 0) best = min(best, (uint64_t)(uint32_t)c << 32 | (uint32_t)j);
    }
    fc = lt_wave_sum(fc);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) best = min(best, wm_shfl_xor(best, off));
    if (lane == 0) {
        int32_t *o = matches + (size_t)t * 8;
        o[4] = (int32_t)fc;
        o[7] = best == WM_NO_KEY ? -1 : members[first + (int)(uint32_t)best];
    }
}

} // namespace

void launch_lattice_track_table(hipStream_t s, int del, int split, const str_er_run_split *splits, const int32_t *first_run, const int32_t *n_of, int n_words, int32_t *tab)
{
    if (n_words > 0) hipLaunchKernelGGL(k_lattice_track_table, dim3((unsigned)((n_words + 63) / 64)), dim3(64), 0, s, del, split, splits, first_run, n_of, n_words, tab);
}

void launch_lattice_track(hipStream_t s, const WmLexDev &lex, const WmParams &p, int split, const str_er_run_split *splits, const uint8_t *run_costs,
                          const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of, int n_words, const int32_t *track_first, const int32_t *track_count,
                          const int32_t *members, const int32_t *slot_track, const int32_t *pslot, int n_members, int n_tracks, int32_t *tab, uint64_t *partial,
                          int32_t *matches, int32_t *mrec, uint8_t *src, int32_t *parts, int32_t *mfree)
{
    launch_lattice_track_table(s, p.del, split, splits, first_run, n_of, n_words, tab);
    const int n_chunks = tm_chunks(lex);
    // (the tracks are the grid's y: at most 65535 a launch)
    for (int t0 = 0; t0 < n_tracks; t0 += 65535) {
        const dim3 grid((unsigned)n_chunks, (unsigned)std::min(65535, n_tracks - t0));
        hipLaunchKernelGGL(k_lattice_track_match, grid, dim3(LT_THREADS), 0, s, lex, p, split, run_costs, piece_costs, n_of, tab, track_first + t0, track_count + t0, members,
                           partial + (size_t)t0 * n_chunks * 2);
    }
    if (n_tracks > 0)
        hipLaunchKernelGGL(k_lattice_track_merge, dim3((unsigned)n_tracks), dim3(64), 0, s, lex, p, n_of, tab, track_first, track_count, members, n_chunks, partial, matches);
    if (n_members > 0)
        hipLaunchKernelGGL(k_lattice_track_members, dim3((unsigned)((n_members + LT_SLOT_WAVES - 1) / LT_SLOT_WAVES)), dim3(64 * LT_SLOT_WAVES), 0, s, lex, p, split, splits,
                           run_costs, piece_costs, first_run, n_of, members, slot_track, pslot, n_members, matches, mrec, src, parts, mfree);
    if (n_tracks > 0) hipLaunchKernelGGL(k_lattice_track_best, dim3((unsigned)n_tracks), dim3(64), 0, s, track_first, track_count, members, mrec, mfree, matches);
}

} // namespace str_er
