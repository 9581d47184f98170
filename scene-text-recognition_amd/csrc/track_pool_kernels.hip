// track_pool_kernels.hip -- the track pool on the device (gfx950): k_pool_add sums, per entry of the lexicon, the edit distances of the
// members a call adds to a slot into the slot's accumulator row, which stays on the device from call to call; k_pool_state_rows /
// _lattice add the members' bands of lengths, free costs and counts to the slot's state; k_pool_read keeps the two smallest (cost,
// index) keys per (slot asked for, chunk) over the entries whose length the slot tries and k_pool_read_final merges the chunks into the
// record; k_pool_join adds rows and states and empties the sources; k_pool_clear empties slots.  Integers only, no atomics and no
// scratch: a workgroup owns the part of the row it writes (the slots of a call are distinct), so the pool holds the same bytes whatever
// the order of the additions.  The rules are stated for the host in track_pool_rules.h; the contract is at str_er_pool_match in str_er.h.
//
// k_pool_add is the member loop of k_track_match (track_match_kernels.hip) and, in lattice mode, of k_lattice_track_match
// (lattice_track_kernels.hip) without the skip of the lengths outside the union of the members' bands: a member added by a later call
// may widen that union, and the entries of the new length must carry this call's members already.  The mask gates the read only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "track_pool_kernels.h"
#include "track_match_device.h"
#include "lattice_track_device.h"

namespace str_er {

namespace {

constexpr int TP_THREADS = 256, TP_WAVES = TP_THREADS / 64;
constexpr int TP_WAVE_GROUPS = TM_CHUNK_GROUPS / TP_WAVES;      // groups of a chunk that one wave takes
constexpr int TP_MASK = 0, TP_FREE = 1, TP_USED = 2, TP_MEMBERS = 3;      // a slot's state
static_assert(TP_WAVE_GROUPS == 4, "the write-back of k_pool_add: sixteen lanes a group, four groups a wave");
static_assert(LT_EROW + LM_SLOTS == LT_TAB_INTS, "the table's row");

// what the members of a call are read from: their cost rows (first_run, n_of per word), or in lattice mode the rows of the runs and
// of the pieces through the words' structure in tab (k_lattice_track_table)
struct TpIn {
    const uint8_t *costs, *piece_costs;
    const int32_t *first_run, *n_of, *tab;
    int            split;
};

// grid (chunks of the whole lexicon, tracks of the call).  The workgroup walks the track's members one at a time, as k_track_match and
// k_lattice_track_match do: the member's rows into LDS, then every wave adds the member's cost of its groups' entries into its lanes'
// accumulators acc[group of the wave][thread] -- every group, whatever its length.  At the end the 64 sums of a group lie back to back
// in LDS, so sixteen lanes add a group to the slot's row with one 16-byte load and store each: a wave's four groups in one instruction.
template <bool LATTICE>
__global__ void __launch_bounds__(TP_THREADS) k_pool_add(WmLexDev lex, WmParams prm, TpIn in, const int32_t *__restrict__ track_first,
                                                         const int32_t *__restrict__ track_count, const int32_t *__restrict__ members,
                                                         const int32_t *__restrict__ slots, TpPoolDev pool)
{
    __shared__ uint8_t ct[(LATTICE ? LM_SLOTS : 32) * WM_ALPHABET];
    __shared__ __attribute__((aligned(16))) int32_t acc[TP_WAVE_GROUPS][TP_THREADS];
    __shared__ int     d0[LM_MAX_NODES + 1];
    __shared__ uint8_t glen[TM_CHUNK_GROUPS];
    const int t = (int)blockIdx.y, chunk = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int first = track_first[t], count = track_count[t];
    const int g0 = chunk * TM_CHUNK_GROUPS, g1 = min(lex.n_groups, g0 + TM_CHUNK_GROUPS);
    if (tid < TM_CHUNK_GROUPS) glen[tid] = (uint8_t)(g0 + tid < g1 ? tm_group_len(lex, g0 + tid) : 0);
#pragma unroll
    for (int gi = 0; gi < TP_WAVE_GROUPS; ++gi) acc[gi][tid] = 0;
    bool any = false;          // (uniform) a usable member was added
    for (int j = 0; j < count; ++j) {
        const int w = __builtin_amdgcn_readfirstlane(members[first + j]);
        if constexpr (LATTICE) {
            const int32_t *T = in.tab + (size_t)w * LT_TAB_INTS;
            const int      N = __builtin_amdgcn_readfirstlane(T[LT_N]);
            if (N > LM_MAX_NODES) continue;          // (uniform: an unusable member)
            const uint32_t S0 = (uint32_t)__builtin_amdgcn_readfirstlane(T[LT_S0]), S1 = (uint32_t)__builtin_amdgcn_readfirstlane(T[LT_S1]);
            const bool     cut = (S0 | S1) != 0;
            const int      MC = N <= 8 ? 8 : N <= 16 ? 16 : 32;
            __syncthreads();          // (the rows of the member before are read)
            if (tid <= LM_MAX_NODES) d0[tid] = T[LT_D0 + tid];
            for (int e = tid; e < (cut ? MC * 4 : MC) * WM_ALPHABET; e += TP_THREADS) {          // a slot without an edge costs 255 (it is never read out)
                const int     k = e / WM_ALPHABET, a = e - k * WM_ALPHABET;
                const int32_t at = T[LT_EROW + (cut ? k : 4 * k)];
                int           v = 255;
                if (at >= 0) {
                    const uint8_t *C = at & LM_PIECE ? in.piece_costs + (size_t)(at & (LM_PIECE - 1)) * WM_ALPHABET : in.costs + (size_t)at * WM_ALPHABET;
                    v = C[a];
                    if (lex.fold) v = min(v, (int)C[wm_partner(a)]);
                }
                ct[e] = (uint8_t)v;
            }
            __syncthreads();
#pragma unroll 1
            for (int gi = 0; gi < TP_WAVE_GROUPS; ++gi) {
                const int gu = __builtin_amdgcn_readfirstlane(g0 + wave + gi * TP_WAVES);
                if (gu >= g1) break;
                const int       len = __builtin_amdgcn_readfirstlane((int)glen[gu - g0]);
                const uint32_t *words = lex.chars + lex.goff[gu] + lane;
                int             c;
                if (cut) {
                    if (MC == 8) c = lm_entry_cost<8>(ct, S0, S1, d0, words, len, N, prm.ins, prm.del, in.split);
                    else if (MC == 16) c = lm_entry_cost<16>(ct, S0, S1, d0, words, len, N, prm.ins, prm.del, in.split);
                    else c = lm_entry_cost<32>(ct, S0, S1, d0, words, len, N, prm.ins, prm.del, in.split);
                } else {
                    if (MC == 8) c = wm_entry_cost<8>(ct, words, len, N, prm.ins, prm.del);
                    else if (MC == 16) c = wm_entry_cost<16>(ct, words, len, N, prm.ins, prm.del);
                    else c = wm_entry_cost<32>(ct, words, len, N, prm.ins, prm.del);
                }
                acc[gi][tid] += c;
            }
        } else {
            const int m = __builtin_amdgcn_readfirstlane(in.n_of[w]);
            if (m > 32) continue;          // (uniform: an unusable member)
            const int      MC = m <= 8 ? 8 : m <= 16 ? 16 : 32;
            const uint8_t *C = in.costs + (size_t)in.first_run[w] * WM_ALPHABET;
            __syncthreads();          // (the rows of the member before are read)
            for (int e = tid; e < MC * WM_ALPHABET; e += TP_THREADS) {          // rows past m cost 255 (they are never read out)
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
            for (int gi = 0; gi < TP_WAVE_GROUPS; ++gi) {
                const int gu = __builtin_amdgcn_readfirstlane(g0 + wave + gi * TP_WAVES);
                if (gu >= g1) break;
                const int       len = __builtin_amdgcn_readfirstlane((int)glen[gu - g0]);
                const uint32_t *words = lex.chars + lex.goff[gu] + lane;
                int             c;
                if (MC == 8) c = wm_entry_cost<8>(ct, words, len, m, prm.ins, prm.del);
                else if (MC == 16) c = wm_entry_cost<16>(ct, words, len, m, prm.ins, prm.del);
                else c = wm_entry_cost<32>(ct, words, len, m, prm.ins, prm.del);
                acc[gi][tid] += c;
            }
        }
        any = true;
    }
    if (!any) return;          // (uniform: nothing to add, the row stays as it is)
    __syncthreads();
    // the group g0 + wave + gi * TP_WAVES has its sums at acc[gi][wave * 64 ..]: the lanes 16 gi .. 16 gi + 15 take four each
    const int gi = lane >> 4, q = (lane & 15) * 4, gu = g0 + wave + gi * TP_WAVES;
    if (gu < g1) {
        const int4 a = *reinterpret_cast<const int4 *>(&acc[gi][wave * 64 + q]);
        int4      *p = reinterpret_cast<int4 *>(pool.acc + (size_t)slots[t] * (size_t)pool.row_ints + (size_t)gu * WM_GROUP + q);
        int4       v = *p;
        v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
        *p = v;
    }
}

// one wave per track of the call: its members' bands of lengths, free costs and counts into the state of its slot (the rules of
// k_track_match_final).  A lane takes every 64th member.
__global__ void __launch_bounds__(64) k_pool_state_rows(WmParams prm, const uint8_t *__restrict__ costs, const int32_t *__restrict__ first_run,
                                                        const int32_t *__restrict__ n_of, const int32_t *__restrict__ track_first,
                                                        const int32_t *__restrict__ track_count, const int32_t *__restrict__ members,
                                                        const int32_t *__restrict__ slots, int32_t *__restrict__ state)
{
    const int t = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int first = track_first[t], count = track_count[t];
    uint32_t  mk = 0, fc = 0, used = 0;
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
    if (lane == 0) {
        int32_t *st = state + (size_t)slots[t] * TP_STATE_INTS;
        st[TP_MASK] = (int32_t)((uint32_t)st[TP_MASK] | mk);
        st[TP_FREE] += (int32_t)fc; st[TP_USED] += (int32_t)used; st[TP_MEMBERS] += count;
    }
}

// one workgroup per track of the call, a wave a member at a time: the free segmentation of the member's runs and its nodes
// (lm_wave_nodes, what k_lattice_track_members and k_lattice_track_best make of them), its lattice band of lengths and the counts
__global__ void __launch_bounds__(TP_THREADS) k_pool_state_lattice(WmParams prm, int split, const str_er_run_split *__restrict__ splits,
                                                                   const uint8_t *__restrict__ run_costs, const uint8_t *__restrict__ piece_costs,
                                                                   const int32_t *__restrict__ first_run, const int32_t *__restrict__ n_of,
                                                                   const int32_t *__restrict__ track_first, const int32_t *__restrict__ track_count,
                                                                   const int32_t *__restrict__ members, const int32_t *__restrict__ slots,
                                                                   int32_t *__restrict__ state)
{
    __shared__ LmWaveLds lds[TP_WAVES];
    __shared__ uint32_t  red[TP_WAVES][3];
    const int t = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int first = track_first[t], count = track_count[t];
    uint32_t  mk = 0, fc = 0, used = 0;          // (uniform per wave)
    for (int j = wave; j < count; j += TP_WAVES) {
        const int w = __builtin_amdgcn_readfirstlane(members[first + j]);
        const int fr = __builtin_amdgcn_readfirstlane(first_run[w]), m = max(0, __builtin_amdgcn_readfirstlane(n_of[w]));
        int       N = 0;
        fc += (uint32_t)lm_wave_nodes(lds[wave], splits, run_costs, piece_costs, fr, m, split, lane, N);
        mk |= lt_len_mask(m, N, prm.band);
        used += N <= LM_MAX_NODES ? 1u : 0u;
    }
    if (lane == 0) { red[wave][0] = mk; red[wave][1] = fc; red[wave][2] = used; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < TP_WAVES; ++v) { mk |= red[v][0]; fc += red[v][1]; used += red[v][2]; }
        int32_t *st = state + (size_t)slots[t] * TP_STATE_INTS;
        st[TP_MASK] = (int32_t)((uint32_t)st[TP_MASK] | mk);
        st[TP_FREE] += (int32_t)fc; st[TP_USED] += (int32_t)used; st[TP_MEMBERS] += count;
    }
}

// grid (chunks of the whole lexicon, slots asked for): the two smallest (cost, index) keys of the chunk over the entries whose length
// the slot tries; the padding of a group (index < 0) never counts
__global__ void __launch_bounds__(TP_THREADS) k_pool_read(WmLexDev lex, TpPoolDev pool, const int32_t *__restrict__ slots, uint64_t *__restrict__ partial)
{
    __shared__ uint64_t wk[TP_WAVES][2];
    const int i = (int)blockIdx.y, chunk = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g0 = chunk * TM_CHUNK_GROUPS, g1 = min(lex.n_groups, g0 + TM_CHUNK_GROUPS);
    const int slot = slots[i];
    const uint32_t mask = (uint32_t)pool.state[(size_t)slot * TP_STATE_INTS + TP_MASK];
    const int32_t *row = pool.acc + (size_t)slot * (size_t)pool.row_ints;
    uint64_t      *out = partial + ((size_t)i * gridDim.x + chunk) * 2;
    uint64_t       k1 = WM_NO_KEY, k2 = WM_NO_KEY;
    if (mask) {          // (uniform)
#pragma unroll 1
        for (int gi = 0; gi < TP_WAVE_GROUPS; ++gi) {
            const int gu = __builtin_amdgcn_readfirstlane(g0 + wave + gi * TP_WAVES);
            if (gu >= g1) break;
            if (!(mask >> (tm_group_len(lex, gu) - 1) & 1u)) continue;          // (a length the slot does not try)
            const int32_t idx = lex.index[(size_t)gu * WM_GROUP + lane];
            if (idx >= 0) wm_add(k1, k2, (uint64_t)(uint32_t)row[(size_t)gu * WM_GROUP + lane] << 32 | (uint32_t)idx);
        }
    }
    tm_wave_best2(k1, k2);
    if (lane == 0) { wk[wave][0] = k1; wk[wave][1] = k2; }
    __syncthreads();
    if (tid == 0) {
        uint64_t b1 = WM_NO_KEY, b2 = WM_NO_KEY;
        for (int v = 0; v < TP_WAVES; ++v) { wm_add(b1, b2, wk[v][0]); wm_add(b1, b2, wk[v][1]); }
        out[0] = b1; out[1] = b2;
    }
}

// one wave per slot asked for: the chunks' pairs merged, the entries tried counted as k_track_match_final counts them, the record
__global__ void __launch_bounds__(64) k_pool_read_final(WmLexDev lex, const int32_t *__restrict__ state, const int32_t *__restrict__ slots, int n_chunks,
                                                        const uint64_t *__restrict__ partial, int32_t *__restrict__ out)
{
    const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
    uint64_t  k1 = WM_NO_KEY, k2 = WM_NO_KEY;
    for (int ch = lane; ch < n_chunks; ch += 64) {
        const uint64_t *p = partial + ((size_t)i * n_chunks + ch) * 2;
        wm_add(k1, k2, p[0]);
        wm_add(k1, k2, p[1]);
    }
    tm_wave_best2(k1, k2);
    if (lane == 0) {
        const int32_t *st = state + (size_t)slots[i] * TP_STATE_INTS;
        const uint32_t mk = (uint32_t)st[TP_MASK];
        int32_t        tried = 0;
        for (int len = 1; len <= 32; ++len)
            if (mk >> (len - 1) & 1u) tried += lex.len_count[len + 1] - lex.len_count[len];
        int32_t *o = out + (size_t)i * 8;
        o[0] = k1 == WM_NO_KEY ? -1 : (int32_t)(uint32_t)k1;
        o[1] = k1 == WM_NO_KEY ? -1 : (int32_t)(k1 >> 32);
        o[2] = k2 == WM_NO_KEY ? -1 : (int32_t)(uint32_t)k2;
        o[3] = k2 == WM_NO_KEY ? -1 : (int32_t)(k2 >> 32);
        o[4] = st[TP_FREE];
        o[5] = tried;
        o[6] = st[TP_USED];
        o[7] = st[TP_MEMBERS];
    }
}

// a thread four entries of the row: dst += the sources, which are zeroed; the first thread merges the states
__global__ void __launch_bounds__(TP_THREADS) k_pool_join(TpPoolDev pool, int dst, const int32_t *__restrict__ srcs, int n_srcs)
{
    const int e = (int)blockIdx.x * TP_THREADS + (int)threadIdx.x;
    if (e < pool.row_ints / 4) {
        int4 *d = reinterpret_cast<int4 *>(pool.acc + (size_t)dst * (size_t)pool.row_ints) + e;
        int4  v = *d;
        for (int k = 0; k < n_srcs; ++k) {
            int4      *sp = reinterpret_cast<int4 *>(pool.acc + (size_t)srcs[k] * (size_t)pool.row_ints) + e;
            const int4 u = *sp;
            v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
            *sp = make_int4(0, 0, 0, 0);
        }
        *d = v;
    }
    if (e == 0) {
        int32_t *D = pool.state + (size_t)dst * TP_STATE_INTS;
        for (int k = 0; k < n_srcs; ++k) {
            int32_t *S = pool.state + (size_t)srcs[k] * TP_STATE_INTS;
            D[TP_MASK] = (int32_t)((uint32_t)D[TP_MASK] | (uint32_t)S[TP_MASK]);
            D[TP_FREE] += S[TP_FREE]; D[TP_USED] += S[TP_USED]; D[TP_MEMBERS] += S[TP_MEMBERS];
            S[TP_MASK] = S[TP_FREE] = S[TP_USED] = S[TP_MEMBERS] = 0;
        }
    }
}

// grid (blocks of the row, slots named): zeroes
__global__ void __launch_bounds__(TP_THREADS) k_pool_clear(TpPoolDev pool, const int32_t *__restrict__ slots)
{
    const int e = (int)blockIdx.x * TP_THREADS + (int)threadIdx.x, slot = slots[blockIdx.y];
    if (e < pool.row_ints / 4) reinterpret_cast<int4 *>(pool.acc + (size_t)slot * (size_t)pool.row_ints)[e] = make_int4(0, 0, 0, 0);
    if (e < TP_STATE_INTS) pool.state[(size_t)slot * TP_STATE_INTS + e] = 0;
}

// (the tracks and the slots asked for are the grid's y: at most 65535 a launch)
template <typename F> void tp_by_y(int n, F launch)
{
    for (int t0 = 0; t0 < n; t0 += 65535) launch(t0, (unsigned)std::min(65535, n - t0));
}

unsigned tp_row_blocks(const TpPoolDev &pool) { return (unsigned)((pool.row_ints / 4 + TP_THREADS - 1) / TP_THREADS); }

} // namespace

void launch_pool_add(hipStream_t s, const WmLexDev &lex, const WmParams &p, const TpPoolDev &pool, const uint8_t *costs, const int32_t *first_run, const int32_t *n_of,
                     const int32_t *track_first, const int32_t *track_count, const int32_t *members, const int32_t *slots, int n_tracks)
{
    if (n_tracks <= 0) return;
    const TpIn in{costs, nullptr, first_run, n_of, nullptr, 0};
    tp_by_y(n_tracks, [&](int t0, unsigned ny) {
        hipLaunchKernelGGL(k_pool_add<false>, dim3((unsigned)tm_chunks(lex), ny), dim3(TP_THREADS), 0, s, lex, p, in, track_first + t0, track_count + t0, members, slots + t0, pool);
    });
    hipLaunchKernelGGL(k_pool_state_rows, dim3((unsigned)n_tracks), dim3(64), 0, s, p, costs, first_run, n_of, track_first, track_count, members, slots, pool.state);
}

void launch_pool_add_lattice(hipStream_t s, const WmLexDev &lex, const WmParams &p, int split, const TpPoolDev &pool, const str_er_run_split *splits,
                             const uint8_t *run_costs, const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of, int n_words, const int32_t *track_first,
                             const int32_t *track_count, const int32_t *members, const int32_t *slots, int n_tracks, int32_t *tab)
{
    if (n_tracks <= 0) return;
    launch_lattice_track_table(s, p.del, split, splits, first_run, n_of, n_words, tab);
    const TpIn in{run_costs, piece_costs, first_run, n_of, tab, split};
    tp_by_y(n_tracks, [&](int t0, unsigned ny) {
        hipLaunchKernelGGL(k_pool_add<true>, dim3((unsigned)tm_chunks(lex), ny), dim3(TP_THREADS), 0, s, lex, p, in, track_first + t0, track_count + t0, members, slots + t0, pool);
    });
    hipLaunchKernelGGL(k_pool_state_lattice, dim3((unsigned)n_tracks), dim3(TP_THREADS), 0, s, p, split, splits, run_costs, piece_costs, first_run, n_of, track_first,
                       track_count, members, slots, pool.state);
}

void launch_pool_read(hipStream_t s, const WmLexDev &lex, const TpPoolDev &pool, const int32_t *slots, int n, uint64_t *partial, int32_t *out)
{
    if (n <= 0) return;
    const int n_chunks = tm_chunks(lex);
    tp_by_y(n, [&](int t0, unsigned ny) {
        hipLaunchKernelGGL(k_pool_read, dim3((unsigned)n_chunks, ny), dim3(TP_THREADS), 0, s, lex, pool, slots + t0, partial + (size_t)t0 * n_chunks * 2);
    });
    hipLaunchKernelGGL(k_pool_read_final, dim3((unsigned)n), dim3(64), 0, s, lex, pool.state, slots, n_chunks, partial, out);
}

void launch_pool_join(hipStream_t s, const TpPoolDev &pool, int dst, const int32_t *srcs, int n_srcs)
{
    if (n_srcs <= 0) return;
    hipLaunchKernelGGL(k_pool_join, dim3(tp_row_blocks(pool)), dim3(TP_THREADS), 0, s, pool, dst, srcs, n_srcs);
}

void launch_pool_clear(hipStream_t s, const TpPoolDev &pool, const int32_t *slots, int n)
{
    if (n <= 0) return;
    tp_by_y(n, [&](int t0, unsigned ny) { hipLaunchKernelGGL(k_pool_clear, dim3(tp_row_blocks(pool), ny), dim3(TP_THREADS), 0, s, pool, slots + t0); });
}

} // namespace str_er
