// track_decode_kernels.hip -- the track decode on the device (gfx950): k_track_decode finds, for every word track, the set median of its
// members' decoder strings under J(s) = lm(s) + the sum of the members' alignment costs, and polishes it by single edits.  Integers
// only, no atomics and no scratch: the output is the same bytes every time.  The rules are stated for the host in
// track_decode_rules.h; the contract is at str_er_track_decode in str_er.h.
//
// One 256-thread workgroup per track, alive over all rounds: the bigram table (the 68-byte rows of k_word_decode), the members' run
// counts and row offsets, the seeds, the current string, the tables, the accumulators and up to 16 KB of rows stay in LDS (60 KB).
//   The recurrence of one member against one string is a wavefront in one wave: lane i holds row i of the table and computes the cell
//     (j, i) at step j + i from its own last value and the last two of lane i - 1 (td_wavefront); l + m + 1 <= 65 steps.
//   The rows of a track whose usable members have at most 16 KB of them (252 rows) are staged once and stay in LDS over all rounds;
//     a larger track stages a member whenever it reads it.
//   Seeds and member costs: a wave takes every fourth member (where the rows are not resident: stages them in a buffer of its own) and
//     runs the wavefront for every seed (for the final string); nothing but a wave-level sync in that loop.
//   A polish round, per usable member: the rows staged by all threads, the prefix table F by wave 0 and the suffix table G by wave 1
//     (the mirrored wavefront), 16-bit cells; then thread t scores the neighbours t, t + 256, ... in O(m) each from F, G and the rows:
//     consecutive threads are consecutive characters a of one position j, so F and G are broadcasts and the row bytes are consecutive.
//     The per-neighbour sums over the members are int32, 17 a thread, in LDS at [q][thread]: in registers the 17 unrolled scoring
//     loops took 252 VGPRs and spilled scalar registers.  lm of a neighbour is lm(s) with the two or three
//     bigrams at the edit exchanged.  The key J << 27 | index << 14 | lm orders by (J, index); its minimum over the workgroup is the
//     step, the same in every thread, and thread 0 edits the string in LDS.
// Every loop is bounded: rounds <= 64, 1024 members, l <= 32.  No workgroup waits for another.
#include <hip/hip_runtime.h>

#include "word_decode_device.h"
#include "track_decode_kernels.h"

namespace str_er {

namespace {

constexpr int TD_THREADS = 256, TD_WAVES = TD_THREADS / 64;
constexpr int TD_MAX_LEN = 32, TD_MAX_SEEDS = 32, TD_MAX_MEMBERS = 1024;
constexpr int TD_SLOT = 2112;                 // bytes of a staged member: up to 32 rows of 65
constexpr int TD_TS = TD_MAX_LEN + 1;         // cells of a table row
constexpr int TD_RES = 16384;                 // bytes of rows that stay in LDS over the rounds
constexpr int TD_DEL_AT = TD_MAX_LEN * WD_ALPHABET, TD_INS_AT = TD_DEL_AT + TD_MAX_LEN, TD_NEIGHBOURS = TD_INS_AT + (TD_MAX_LEN + 1) * WD_ALPHABET;
constexpr int TD_PER_THREAD = (TD_NEIGHBOURS + TD_THREADS - 1) / TD_THREADS;
constexpr uint64_t TD_NO_KEY = ~0ull;
static_assert(TD_SLOT >= TD_MAX_LEN * WD_ALPHABET && TD_PER_THREAD == 17, "track decode layout");

// D[m][l] of the matcher's recurrence for the m rows at `rows` (LDS) against the l labels at s (LDS), in every lane; called by a whole
// wave.  Lane i computes the cell (j, i) at step j + i.  REV: the mirrored recurrence, the labels from the end against the rows from
// the end.  STORE: every cell goes into tab, F[j][i] at j * TD_TS + i, and mirrored G[j][i] at the same place.
template <bool REV, bool STORE>
__device__ __forceinline__ int td_wavefront(const uint8_t *rows, int m, const uint8_t *s, int l, int ins, int del, uint16_t *tab, int lane)
{
    int cur = 0, prev = 0;
    for (int t = 0; t <= l + m; ++t) {
        const int a = __shfl_up(cur, 1, 64), b = __shfl_up(prev, 1, 64);
        const int j = t - lane;
        int       v = cur;
        if (lane <= m && j >= 0 && j <= l) {
            if (j == 0) v = lane * del;
            else if (lane == 0) v = j * ins;
            else {
                const int c = REV ? rows[(m - lane) * WD_ALPHABET + s[l - j]] : rows[(lane - 1) * WD_ALPHABET + s[j - 1]];
                v = min(b + c, min(a + del, cur + ins));
            }
            if (STORE) tab[REV ? (l - j) * TD_TS + (m - lane) : j * TD_TS + lane] = (uint16_t)v;
        }
        prev = cur;
        cur = v;
    }
    return __shfl(cur, m, 64);
}

__device__ __forceinline__ uint64_t td_wave_min(uint64_t k)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)k, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), off, 64);
        const uint64_t o = (uint64_t)hi << 32 | lo;
        k = o < k ? o : k;
    }
    return k;
}

// the rows of a member into LDS, by n threads of which this is thread t
__device__ __forceinline__ void td_stage(uint8_t *to, const uint8_t *__restrict__ C, int m, int t, int n)
{
    for (int e = t; e < m * WD_ALPHABET; e += n) to[e] = C[e];
}

// the cost of the labels before j, then a (a < 0: none), then the labels from g on: F's row j and G's row g meet at any row i, the
// label a on a row of its own or inserted
__device__ __forceinline__ int td_joined(const uint16_t *Fj, const uint16_t *Gg, const uint8_t *rows, int m, int a, int ins)
{
    if (a < 0) {
        int best = (int)Fj[m] + (int)Gg[m];
#pragma unroll 4
        for (int i = 0; i < m; ++i) best = min(best, (int)Fj[i] + (int)Gg[i]);
        return best;
    }
    int best = (int)Fj[m] + ins + (int)Gg[m];
#pragma unroll 4
    for (int i = 0; i < m; ++i) best = min(best, (int)Fj[i] + min(ins + (int)Gg[i], (int)rows[i * WD_ALPHABET + a] + (int)Gg[i + 1]));
    return best;
}

// what the neighbour x is: the labels before j stay, then a (-1: none), then the labels from g on (INS: g = j); x < TD_NEIGHBOURS
__device__ __forceinline__ void td_neighbour(int x, int &j, int &a, int &g)
{
    if (x < TD_DEL_AT) { j = x / WD_ALPHABET; a = x - j * WD_ALPHABET; g = j + 1; }
    else if (x < TD_INS_AT) { j = x - TD_DEL_AT; a = -1; g = j + 1; }
    else { const int y = x - TD_INS_AT; j = y / WD_ALPHABET; a = y - j * WD_ALPHABET; g = j; }
}

__global__ void __launch_bounds__(TD_THREADS) k_track_decode(const uint8_t *__restrict__ bigram, int ins, int del, int rounds, const uint8_t *__restrict__ costs,
                                                             const int32_t *__restrict__ first_run, const int32_t *__restrict__ n_of,
                                                             const int32_t *__restrict__ dec, const uint8_t *__restrict__ dchars,
                                                             const int32_t *__restrict__ track_first, const int32_t *__restrict__ track_count,
                                                             const int32_t *__restrict__ members, int32_t *__restrict__ out, uint8_t *__restrict__ chars,
                                                             int32_t *__restrict__ member_cost)
{
    __shared__ __attribute__((aligned(16))) uint8_t Bs[WD_STATES * WD_ROW];
    __shared__ __attribute__((aligned(16))) uint8_t stage[TD_WAVES][TD_SLOT];
    __shared__ uint16_t F[TD_TS * TD_TS], G[TD_TS * TD_TS];
    __shared__ int32_t  mfirst[TD_MAX_MEMBERS];
    __shared__ uint8_t  mlen[TD_MAX_MEMBERS], mseed[TD_MAX_MEMBERS];          // run count (255: unusable), length of the decoder string if it can be a seed (else 0)
    __shared__ uint8_t  seeds[TD_MAX_SEEDS][TD_MAX_LEN];
    __shared__ int16_t  seed_slot[TD_MAX_SEEDS];
    __shared__ int32_t  seed_lm[TD_MAX_SEEDS], seed_a[TD_WAVES][TD_MAX_SEEDS];
    __shared__ uint8_t  str[TD_MAX_LEN + 4];
    __shared__ uint64_t wk[TD_WAVES];
    __shared__ int32_t  acc[TD_PER_THREAD][TD_THREADS];
    __shared__ int32_t  wcount[TD_WAVES][2];
    __shared__ __attribute__((aligned(16))) uint8_t res[TD_RES];
    __shared__ uint16_t roff[TD_MAX_MEMBERS];          // where a usable member's rows start in res
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int first = track_first[g], count = min(track_count[g], TD_MAX_MEMBERS);
    for (int t = tid; t < WD_STATES * WD_ROW; t += TD_THREADS) {
        const int a = t / WD_ROW, b = t - a * WD_ROW;
        Bs[t] = b < WD_STATES ? bigram[a * WD_STATES + b] : (uint8_t)0;
    }
    int used = 0;
    for (int k = tid; k < count; k += TD_THREADS) {
        const int w = members[first + k], m = n_of[w], nc = dec[(size_t)w * 6 + 2];
        const bool ok = m <= TD_MAX_LEN;
        mfirst[k] = first_run[w];
        mlen[k] = (uint8_t)(ok ? max(m, 0) : 255);
        mseed[k] = (uint8_t)(ok && nc >= 1 && nc <= TD_MAX_LEN ? nc : 0);
        used += ok ? 1 : 0;
    }
    if (tid < TD_MAX_SEEDS) {
#pragma unroll
        for (int v = 0; v < TD_WAVES; ++v) seed_a[v][tid] = 0;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) used += __shfl_xor(used, off, 64);
    if (lane == 0) wcount[wave][0] = used;
    __syncthreads();
    used = 0;
#pragma unroll
    for (int v = 0; v < TD_WAVES; ++v) used += wcount[v][0];
    // the seeds: the first 32 slots with a string of 1 .. 32 labels, by wave 0
    if (wave == 0) {
        int n = 0;
        for (int base = 0; base < count && n < TD_MAX_SEEDS; base += 64) {
            const int      k = base + lane;
            const bool     q = k < count && mseed[k] > 0;
            const uint64_t mask = __ballot(q);
            const int      rank = n + __popcll(mask & ((1ull << lane) - 1ull));
            if (q && rank < TD_MAX_SEEDS) seed_slot[rank] = (int16_t)k;
            n += __popcll(mask);
        }
        if (lane == 0) wcount[0][1] = min(n, TD_MAX_SEEDS);
    }
    if (tid == 64) {          // ... and whether the usable members' rows fit res, with their places, by one thread of wave 1
        int at = 0, fits = 1;
        for (int k = 0; k < count; ++k) {
            const int m = (int)mlen[k];
            if (m > TD_MAX_LEN) continue;
            if (at + m * WD_ALPHABET > TD_RES) { fits = 0; break; }
            roff[k] = (uint16_t)at;
            at += m * WD_ALPHABET;
        }
        wcount[1][1] = fits;
    }
    __syncthreads();
    const int  n_seeds = wcount[0][1];
    const bool resident = wcount[1][1] != 0;          // (uniform)
    int32_t  *o = out + (size_t)g * 8;
    if (n_seeds == 0) {          // (uniform) not decoded
        if (tid == 0) { o[0] = -1; o[1] = -1; o[2] = 0; o[3] = 0; o[4] = 0; o[5] = used; o[6] = -1; o[7] = -1; }
        if (tid < TD_MAX_LEN) chars[(size_t)g * TD_MAX_LEN + tid] = 0xFF;
        for (int k = tid; k < count; k += TD_THREADS) member_cost[first + k] = -1;
        return;
    }
    if (resident)
        for (int k = wave; k < count; k += TD_WAVES)
            if ((int)mlen[k] <= TD_MAX_LEN) td_stage(res + roff[k], costs + (size_t)mfirst[k] * WD_ALPHABET, (int)mlen[k], lane, 64);
    for (int e = tid; e < n_seeds * TD_MAX_LEN; e += TD_THREADS) {
        const int sd = e >> 5, pos = e & 31, k = seed_slot[sd];
        seeds[sd][pos] = pos < (int)mseed[k] ? dchars[(size_t)members[first + k] * 64 + pos] : (uint8_t)0;
    }
    __syncthreads();
    if (tid < n_seeds) {
        const uint8_t *sv = seeds[tid];
        const int      l = (int)mseed[seed_slot[tid]];
        int32_t        c = (int32_t)Bs[WD_E * WD_ROW + sv[0]] + (int32_t)Bs[sv[l - 1] * WD_ROW + WD_E];
        for (int j = 0; j + 1 < l; ++j) c += (int32_t)Bs[sv[j] * WD_ROW + sv[j + 1]];
        seed_lm[tid] = c;
    }
    // J of every seed: a wave a member, its own staging buffer
    uint8_t *mine = stage[wave];
    for (int k = wave; k < count; k += TD_WAVES) {
        const int m = (int)mlen[k];
        if (m > TD_MAX_LEN) continue;          // (uniform in the wave)
        const uint8_t *R = mine;
        if (resident) R = res + roff[k];
        else {
            wd_wave_sync();
            td_stage(mine, costs + (size_t)mfirst[k] * WD_ALPHABET, m, lane, 64);
            wd_wave_sync();
        }
        for (int sd = 0; sd < n_seeds; ++sd) {
            const int c = td_wavefront<false, false>(R, m, seeds[sd], (int)mseed[seed_slot[sd]], ins, del, nullptr, lane);
            if (lane == 0) seed_a[wave][sd] += c;
        }
    }
    __syncthreads();
    if (wave == 0) {
        uint64_t key = TD_NO_KEY;
        if (lane < n_seeds) {
            int32_t J = seed_lm[lane];
#pragma unroll
            for (int v = 0; v < TD_WAVES; ++v) J += seed_a[v][lane];
            key = (uint64_t)(uint32_t)J << 8 | (uint32_t)lane;
        }
        key = td_wave_min(key);
        if (lane == 0) wk[0] = key;
    }
    __syncthreads();
    const int seed = (int)(wk[0] & 255u);
    int32_t   J = (int32_t)(wk[0] >> 8), lmS = seed_lm[seed];
    int       l = (int)mseed[seed_slot[seed]];
    const int32_t seed_cost = J, seed_member = members[first + seed_slot[seed]];
    if (tid < TD_MAX_LEN) str[tid] = seeds[seed][tid];
    __syncthreads();
    int n_edits = 0, converged = 0;
    for (int round = 1; round <= rounds; ++round) {
        // which of the thread's neighbours exist at this length
        uint32_t live = 0;
#pragma unroll
        for (int q = 0; q < TD_PER_THREAD; ++q) {
            const int x = tid + q * TD_THREADS;
            bool      ok = false;
            if (x < TD_DEL_AT) ok = x < l * WD_ALPHABET;
            else if (x < TD_INS_AT) ok = l > 1 && x - TD_DEL_AT < l;
            else if (x < TD_NEIGHBOURS) ok = l < TD_MAX_LEN && x - TD_INS_AT < (l + 1) * WD_ALPHABET;
            live |= ok ? 1u << q : 0u;
            acc[q][tid] = 0;
        }
        for (int k = 0; k < count; ++k) {
            const int m = (int)mlen[k];
            if (m > TD_MAX_LEN) continue;          // (uniform)
            __syncthreads();          // (the rows and tables of the member before are read)
            const uint8_t *rows = stage[0];
            if (resident) rows = res + roff[k];
            else {
                td_stage(stage[0], costs + (size_t)mfirst[k] * WD_ALPHABET, m, tid, TD_THREADS);
                __syncthreads();
            }
            if (wave == 0) td_wavefront<false, true>(rows, m, str, l, ins, del, F, lane);
            else if (wave == 1) td_wavefront<true, true>(rows, m, str, l, ins, del, G, lane);
            __syncthreads();
            for (uint32_t todo = live; todo; todo &= todo - 1u) {
                const int q = __ffs((int)todo) - 1;
                int       j, a, gg;
                td_neighbour(tid + q * TD_THREADS, j, a, gg);
                acc[q][tid] += td_joined(F + j * TD_TS, G + gg * TD_TS, rows, m, a, ins);
            }
        }
        uint64_t key = TD_NO_KEY;
        for (uint32_t todo = live; todo; todo &= todo - 1u) {
            const int q = __ffs((int)todo) - 1;
            int       j, a, gg;
            td_neighbour(tid + q * TD_THREADS, j, a, gg);
            const int p = j > 0 ? (int)str[j - 1] : WD_E;
            int32_t   lm = lmS;
            if (gg == j) {          // INS
                const int nx = j < l ? (int)str[j] : WD_E;
                lm += (int32_t)Bs[p * WD_ROW + a] + (int32_t)Bs[a * WD_ROW + nx] - (int32_t)Bs[p * WD_ROW + nx];
            } else {
                const int old = (int)str[j], nx = j + 1 < l ? (int)str[j + 1] : WD_E;
                lm -= (int32_t)Bs[p * WD_ROW + old] + (int32_t)Bs[old * WD_ROW + nx];
                lm += a >= 0 ? (int32_t)Bs[p * WD_ROW + a] + (int32_t)Bs[a * WD_ROW + nx] : (int32_t)Bs[p * WD_ROW + nx];
            }
            const uint64_t kq = (uint64_t)(uint32_t)(acc[q][tid] + lm) << 27 | (uint64_t)(uint32_t)(tid + q * TD_THREADS) << 14 | (uint32_t)lm;
            key = kq < key ? kq : key;
        }
        key = td_wave_min(key);
        if (lane == 0) wk[wave] = key;
        __syncthreads();
        key = wk[0];
#pragma unroll
        for (int v = 1; v < TD_WAVES; ++v) key = wk[v] < key ? wk[v] : key;
        const int32_t Jb = (int32_t)(key >> 27);
        if (key == TD_NO_KEY || Jb >= J) { converged = 1; break; }          // (uniform)
        const int x = (int)(key >> 14 & 8191u);
        int       nl = l;
        if (x < TD_DEL_AT) {
            if (tid == 0) str[x / WD_ALPHABET] = (uint8_t)(x % WD_ALPHABET);
        } else if (x < TD_INS_AT) {
            if (tid == 0)
                for (int q = x - TD_DEL_AT; q + 1 < l; ++q) str[q] = str[q + 1];
            nl = l - 1;
        } else {
            const int y = x - TD_INS_AT, j = y / WD_ALPHABET;
            if (tid == 0) {
                for (int q = l; q > j; --q) str[q] = str[q - 1];
                str[j] = (uint8_t)(y - j * WD_ALPHABET);
            }
            nl = l + 1;
        }
        l = nl; J = Jb; lmS = (int32_t)(key & 16383u);
        ++n_edits;
        __syncthreads();          // (the string as thread 0 left it; wk is read)
    }
    __syncthreads();
    // the members' own costs for the string: a wave a member again
    for (int k = wave; k < count; k += TD_WAVES) {
        const int m = (int)mlen[k];
        int       c = -1;
        if (m <= TD_MAX_LEN) {          // (uniform in the wave)
            const uint8_t *R = mine;
            if (resident) R = res + roff[k];
            else {
                wd_wave_sync();
                td_stage(mine, costs + (size_t)mfirst[k] * WD_ALPHABET, m, lane, 64);
                wd_wave_sync();
            }
            c = td_wavefront<false, false>(R, m, str, l, ins, del, nullptr, lane);
        }
        if (lane == 0) member_cost[first + k] = c;
    }
    if (tid == 0) { o[0] = J; o[1] = seed_cost; o[2] = l; o[3] = n_edits; o[4] = converged; o[5] = used; o[6] = seed_member; o[7] = lmS; }
    if (tid < TD_MAX_LEN) chars[(size_t)g * TD_MAX_LEN + tid] = tid < l ? str[tid] : (uint8_t)0xFF;
}

} // namespace

void launch_track_decode(hipStream_t s, const uint8_t *bigram, int ins, int del, int rounds, const uint8_t *costs, const int32_t *first_run, const int32_t *n_of,
                         const void *dec, const uint8_t *dchars, const int32_t *track_first, const int32_t *track_count, const int32_t *members, int n_tracks,
                         void *out, uint8_t *chars, int32_t *member_cost)
{
    if (n_tracks <= 0) return;
    hipLaunchKernelGGL(k_track_decode, dim3((unsigned)n_tracks), dim3(TD_THREADS), 0, s, bigram, ins, del, rounds, costs, first_run, n_of,
                       static_cast<const int32_t *>(dec), dchars, track_first, track_count, members, static_cast<int32_t *>(out), chars, member_cost);
}

} // namespace str_er
