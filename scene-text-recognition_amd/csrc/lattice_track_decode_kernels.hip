// lattice_track_decode_kernels.hip -- the track decode over the members' piece lattices on the device (gfx950): k_lattice_track_decode
// finds, for every word track, the seed with the smallest J(s) = lm(s) + the sum of the members' lattice edit distances L_i(s) and
// polishes it by single edits with every member's segmentation free; k_lattice_track_decode_members then runs, a wave a slot of the
// member array, the table and the backtrack of the final string (lm_wave_nodes, lm_wave_labels, lm_wave_store of
// lattice_match_device.h).  Integers only, no atomics and no scratch: the output is the same bytes every time.  The rules are stated
// for the host in lattice_track_decode_rules.h; the contract is at str_er_lattice_track_decode in str_er.h.
//
// k_lattice_track_decode is built like k_track_decode (track_decode_kernels.hip): one 256-thread workgroup per track, alive over all
// rounds, with the bigram table, the members, the seeds, the string, the tables and the accumulators in LDS.  What differs:
//   A member is its lattice.  Its structure (N, the local index of every node) comes from k_lattice_track_table's row of the word; a
//     wave turns it into the edge list of the member (ltd_meta: from node, to node, whether the edge pays SPLIT, a node's first edge),
//     and the member's rows in LDS are its edges in that order: at most 80 of 65 bytes, 5200 bytes (2112 in the track decode).
//   The tables run over nodes: F[j][n] the first j labels with the path at node n, G[g][n] the labels from g on from node n to N.  A
//     node has up to 4 incoming edges, so a lane is a label position and the wave walks the nodes (at most 32 steps) with the columns of
//     the last four nodes in registers, those of the lane's neighbour beside them; the INS chain is a prefix minimum over the lanes
//     (ltd_forward).  G is the mirror: the edges that leave a node and a suffix minimum (ltd_backward).
//     16-bit cells: a cell is at most the cost of inserting every label and deleting every node over its shortest edges,
//     32 * 255 + 32 * (255 + 255) = 24480 < 65536.
//   A neighbour "labels before j, then a, then labels from g on" costs min over n of F[j][n] + G[g][n] without a, and with a the smaller
//     of min over n of F[j][n] + INS + G[g][n] and min over the edges (f -> n) of F[j][f] + C_e[a] + s_e + G[g][n] (ltd_joined).
//   All four waves build tables: a polish round takes the usable members two at a time, waves 0 / 1 make F / G of the first and waves
//     2 / 3 those of the second, then every thread scores its neighbours on both.
//   LDS: 44 KB of tables and lists and a pool of 512 edge rows (33280 bytes), 77608 bytes in all, so that two workgroups fit the 160 KB of
//     a CU.  A track whose usable members have at most 512 edges keeps their rows in the pool over all rounds; a larger track uses the
//     front of the pool as four staging buffers of 5200 bytes and stages a member whenever it reads it.
// Every loop is bounded: rounds <= 64, 1024 members, l <= 32, N <= 32.  No workgroup waits for another.
#include <hip/hip_runtime.h>

#include "word_decode_device.h"
#include "lattice_track_device.h"
#include "lattice_track_decode_kernels.h"

namespace str_er {

namespace {

constexpr int LTD_THREADS = 256, LTD_WAVES = LTD_THREADS / 64;
constexpr int LTD_MAX_LEN = 32, LTD_MAX_SEEDS = 32, LTD_MAX_MEMBERS = 1024;
constexpr int LTD_MAX_EDGES = 80;                        // of a member: 8 runs of 4 atoms with 10 edges each
constexpr int LTD_SLOT = LTD_MAX_EDGES * WD_ALPHABET;    // bytes of a staged member
constexpr int LTD_TS = LM_MAX_NODES + 1;                 // cells of a table row: the nodes 0 .. 32
constexpr int LTD_RES_EDGES = 512;                       // edge rows that stay in LDS over the rounds
constexpr int LTD_POOL = LTD_RES_EDGES * WD_ALPHABET;
constexpr int LTD_DEL_AT = LTD_MAX_LEN * WD_ALPHABET, LTD_INS_AT = LTD_DEL_AT + LTD_MAX_LEN, LTD_NEIGHBOURS = LTD_INS_AT + (LTD_MAX_LEN + 1) * WD_ALPHABET;
constexpr int LTD_PER_THREAD = (LTD_NEIGHBOURS + LTD_THREADS - 1) / LTD_THREADS;
constexpr int LTD_BIG = 1 << 28;
constexpr uint64_t LTD_NO_KEY = ~0ull;
static_assert(LTD_POOL >= LTD_WAVES * LTD_SLOT && LTD_PER_THREAD == 17 && WD_ALPHABET == WM_ALPHABET, "lattice track decode layout");

// the edge list of one member: the edge e = from | to << 8 | (pays SPLIT) << 16, the edges into a node back to back in the order of their
// span d = 1 .. jl; first[n] the first edge into the node n >= 1, jl[n] their number (0 past N)
struct LtdMeta {
    uint32_t edge[LTD_MAX_EDGES];
    uint8_t  first[LM_MAX_NODES + 8], jl[LM_MAX_NODES + 8];
    int32_t  N, E;
};

// the number of edges of a word with N <= 32 nodes from its structure words: every node has jl = field + 1 of them
__device__ __forceinline__ int ltd_edges(int N, uint32_t S0, uint32_t S1)
{
    return N + __popc(S0 & 0x55555555u) + 2 * __popc(S0 & 0xAAAAAAAAu) + __popc(S1 & 0x55555555u) + 2 * __popc(S1 & 0xAAAAAAAAu);
}

// the edge list of the word with the table row T into M, by a whole wave (the caller syncs before M is read); N <= 32
__device__ __forceinline__ void ltd_meta(LtdMeta &M, const int32_t *__restrict__ T, int lane)
{
    const int      N = __builtin_amdgcn_readfirstlane(T[LT_N]);
    const uint32_t S0 = (uint32_t)__builtin_amdgcn_readfirstlane(T[LT_S0]), S1 = (uint32_t)__builtin_amdgcn_readfirstlane(T[LT_S1]);
    const int      n = lane;
    const int      jl = n >= 1 && n <= N ? (int)((n <= 16 ? S0 : S1) >> (2 * ((n - 1) & 15)) & 3u) + 1 : 0;
    int            incl = jl;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    const int eb = incl - jl;
    if (n < LM_MAX_NODES + 8) { M.first[n] = (uint8_t)min(eb, LTD_MAX_EDGES); M.jl[n] = (uint8_t)jl; }
    for (int d = 1; d <= jl; ++d)
        if (eb + d <= LTD_MAX_EDGES && d <= n) M.edge[eb + d - 1] = (uint32_t)(n - d) | (uint32_t)n << 8 | (d < jl ? 1u << 16 : 0u);
    if (lane == 0) { M.N = N; M.E = min(ltd_edges(N, S0, S1), LTD_MAX_EDGES); }
}

// the rows of the member's edges into LDS, in the order of M, by n threads of which this is thread t
__device__ __forceinline__ void ltd_stage(uint8_t *to, const LtdMeta &M, const int32_t *__restrict__ T, const uint8_t *__restrict__ run_costs,
                                          const uint8_t *__restrict__ piece_costs, int t, int n)
{
    const int bytes = M.E * WD_ALPHABET;
    for (int x = t; x < bytes; x += n) {
        const int      e = x / WD_ALPHABET, a = x - e * WD_ALPHABET;
        const uint32_t ed = M.edge[e];
        const int      to_n = (int)(ed >> 8 & 0xFFu), d = to_n - (int)(ed & 0xFFu);
        const int32_t  at = T[LT_EROW + (to_n - 1) * 4 + d - 1];
        if (at < 0) { to[x] = 255; continue; }          // (a slot without an edge: the list and the table would disagree)
        const uint8_t *C = at & LM_PIECE ? piece_costs + (size_t)(at & (LM_PIECE - 1)) * WD_ALPHABET : run_costs + (size_t)at * WD_ALPHABET;
        to[x] = C[a];
    }
}

// one edge into the node n from D_ nodes back: O_ the column of that node at the lane's label, P_ at the label before
#define LTD_IN(D_, O_, P_)                                                                        \
    {                                                                                             \
        const int pen = D_ < jl ? split : 0;                                                      \
        const int c = (int)rows[(eb + D_ - 1) * WD_ALPHABET + a];                                 \
        X = min(X, O_ + del + pen);                                                               \
        if (j >= 1) X = min(X, P_ + c + pen);                                                     \
    }

// L(s) = D[N][l] of the lattice recurrence for the member with the edge list M and the rows `rows` (LDS) against the l labels at s
// (LDS), in every lane; called by a whole wave.  Lane j holds the label position j and walks the nodes.  STORE: every cell goes into
// tab, F[j][n] at j * LTD_TS + n.
template <bool STORE>
__device__ __forceinline__ int ltd_forward(const uint8_t *rows, const LtdMeta &M, const uint8_t *s, int l, int ins, int del, int split, uint16_t *tab, int lane)
{
    const int j = lane, N = __builtin_amdgcn_readfirstlane(M.N);
    const int a = j >= 1 && j <= l ? (int)s[j - 1] : 0;
    int       o1 = j * ins, o2 = 0, o3 = 0, o4 = 0;          // the columns of the nodes n - 1 .. n - 4 at the label j
    int       p1 = __shfl_up(o1, 1, 64), p2 = 0, p3 = 0, p4 = 0;          // ... and at the label j - 1
    if (STORE && j <= l) tab[j * LTD_TS] = (uint16_t)o1;
    for (int n = 1; n <= N; ++n) {
        const int jl = __builtin_amdgcn_readfirstlane((int)M.jl[n]), eb = __builtin_amdgcn_readfirstlane((int)M.first[n]);
        int       X = LTD_BIG;
        LTD_IN(1, o1, p1)
        if (jl >= 2) {          // (uniform)
            LTD_IN(2, o2, p2)
            if (jl >= 3) {
                LTD_IN(3, o3, p3)
                if (jl >= 4) LTD_IN(4, o4, p4)
            }
        }
        int v = X - j * ins;          // the INS chain: a prefix minimum over the lanes
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(v, off, 64);
            if (lane >= off) v = min(v, o);
        }
        v += j * ins;
        if (STORE && j <= l) tab[j * LTD_TS + n] = (uint16_t)v;
        o4 = o3; o3 = o2; o2 = o1; o1 = v;
        p4 = p3; p3 = p2; p2 = p1; p1 = __shfl_up(v, 1, 64);
    }
    return __shfl(o1, l, 64);
}
#undef LTD_IN

// one edge that leaves the node n, D_ nodes on (uniform: whether it exists): Q_ the column of that node at the lane's label, R_ at the next
#define LTD_OUT(D_, Q_, R_)                                                                       \
    if (n + D_ <= N) {                                                                            \
        const int jt = __builtin_amdgcn_readfirstlane((int)M.jl[n + D_]);                         \
        if (D_ <= jt) {                                                                           \
            const int eb = __builtin_amdgcn_readfirstlane((int)M.first[n + D_]);                  \
            const int pen = D_ < jt ? split : 0;                                                  \
            const int c = (int)rows[(eb + D_ - 1) * WD_ALPHABET + a];                             \
            Y = min(Y, Q_ + del + pen);                                                           \
            if (g < l) Y = min(Y, R_ + c + pen);                                                  \
        }                                                                                         \
    }

// the mirror: G[g][n], the labels from g on from the node n to N, into tab at g * LTD_TS + n; lane g holds the label position g.
// Returns G[0][0] = L(s) in every lane.
__device__ __forceinline__ int ltd_backward(const uint8_t *rows, const LtdMeta &M, const uint8_t *s, int l, int ins, int del, int split, uint16_t *tab, int lane)
{
    const int g = lane, N = __builtin_amdgcn_readfirstlane(M.N);
    const int a = g < l ? (int)s[g] : 0;
    int       q1 = g <= l ? (l - g) * ins : LTD_BIG, q2 = LTD_BIG, q3 = LTD_BIG, q4 = LTD_BIG;          // the columns of the nodes n + 1 .. n + 4 at the label g
    int       r1 = __shfl_down(q1, 1, 64), r2 = LTD_BIG, r3 = LTD_BIG, r4 = LTD_BIG;                    // ... and at the label g + 1
    if (g <= l) tab[g * LTD_TS + N] = (uint16_t)q1;
    for (int n = N - 1; n >= 0; --n) {
        int Y = LTD_BIG;
        LTD_OUT(1, q1, r1)
        LTD_OUT(2, q2, r2)
        LTD_OUT(3, q3, r3)
        LTD_OUT(4, q4, r4)
        int v = g <= l ? Y + g * ins : LTD_BIG;          // the INS chain: a suffix minimum over the lanes
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_down(v, off, 64);
            if (lane + off < 64) v = min(v, o);
        }
        v = g <= l ? v - g * ins : LTD_BIG;
        if (g <= l) tab[g * LTD_TS + n] = (uint16_t)v;
        q4 = q3; q3 = q2; q2 = q1; q1 = v;
        r4 = r3; r3 = r2; r2 = r1; r1 = __shfl_down(v, 1, 64);
    }
    return __shfl(q1, 0, 64);
}
#undef LTD_OUT

__device__ __forceinline__ uint64_t ltd_wave_min(uint64_t k)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)k, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), off, 64);
        const uint64_t o = (uint64_t)hi << 32 | lo;
        k = o < k ? o : k;
    }
    return k;
}

// the cost of the labels before j, then a (a < 0: none), then the labels from g on: F's row j and G's row g meet at any node, the label
// a inserted there or read from an edge
__device__ __forceinline__ int ltd_joined(const uint16_t *Fj, const uint16_t *Gg, const uint8_t *rows, const LtdMeta &M, int a, int ins, int split)
{
    const int N = M.N, E = M.E;
    int       best = (int)Fj[0] + (int)Gg[0];
#pragma unroll 4
    for (int n = 1; n <= N; ++n) best = min(best, (int)Fj[n] + (int)Gg[n]);
    if (a < 0) return best;
    best += ins;
#pragma unroll 4
    for (int e = 0; e < E; ++e) {
        const uint32_t ed = M.edge[e];
        best = min(best, (int)Fj[ed & 0xFFu] + (int)rows[e * WD_ALPHABET + a] + (ed >> 16 ? split : 0) + (int)Gg[ed >> 8 & 0xFFu]);
    }
    return best;
}

// what the neighbour x is: the labels before j stay, then a (-1: none), then the labels from g on (INS: g = j); x < LTD_NEIGHBOURS
__device__ __forceinline__ void ltd_neighbour(int x, int &j, int &a, int &g)
{
    if (x < LTD_DEL_AT) { j = x / WD_ALPHABET; a = x - j * WD_ALPHABET; g = j + 1; }
    else if (x < LTD_INS_AT) { j = x - LTD_DEL_AT; a = -1; g = j + 1; }
    else { const int y = x - LTD_INS_AT; j = y / WD_ALPHABET; a = y - j * WD_ALPHABET; g = j; }
}

__global__ void __launch_bounds__(LTD_THREADS) k_lattice_track_decode(const uint8_t *__restrict__ bigram, int ins, int del, int rounds, int split,
                                                                      const uint8_t *__restrict__ run_costs, const uint8_t *__restrict__ piece_costs,
                                                                      const int32_t *__restrict__ tab, const int32_t *__restrict__ dec,
                                                                      const uint8_t *__restrict__ dchars, const int32_t *__restrict__ track_first,
                                                                      const int32_t *__restrict__ track_count, const int32_t *__restrict__ members,
                                                                      int32_t *__restrict__ out, uint8_t *__restrict__ chars)
{
    __shared__ __attribute__((aligned(16))) uint8_t Bs[WD_STATES * WD_ROW];
    __shared__ __attribute__((aligned(16))) uint8_t pool[LTD_POOL];          // the resident rows, or at its front a staging buffer per wave
    __shared__ uint16_t F[2][LTD_TS * LTD_TS], G[2][LTD_TS * LTD_TS];
    __shared__ LtdMeta  meta[LTD_WAVES];
    __shared__ int32_t  mword[LTD_MAX_MEMBERS];
    __shared__ uint8_t  medges[LTD_MAX_MEMBERS], mseed[LTD_MAX_MEMBERS];      // edges (255: unusable), length of the lattice decoder's string if it can be a seed (else 0)
    __shared__ uint16_t roff[LTD_MAX_MEMBERS], ulist[LTD_MAX_MEMBERS];        // where a usable member's rows start in the pool (in rows); the usable slots in order
    __shared__ uint8_t  seeds[LTD_MAX_SEEDS][LTD_MAX_LEN];
    __shared__ int16_t  seed_slot[LTD_MAX_SEEDS];
    __shared__ int32_t  seed_lm[LTD_MAX_SEEDS], seed_a[LTD_WAVES][LTD_MAX_SEEDS];
    __shared__ uint8_t  str[LTD_MAX_LEN + 4];
    __shared__ uint64_t wk[LTD_WAVES];
    __shared__ int32_t  acc[LTD_PER_THREAD][LTD_THREADS];
    __shared__ int32_t  wcount[4];          // seeds, usable members, whether the rows are resident
    const int t_ = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int first = track_first[t_], count = min(track_count[t_], LTD_MAX_MEMBERS);
    for (int t = tid; t < WD_STATES * WD_ROW; t += LTD_THREADS) {
        const int a = t / WD_ROW, b = t - a * WD_ROW;
        Bs[t] = b < WD_STATES ? bigram[a * WD_STATES + b] : (uint8_t)0;
    }
    for (int k = tid; k < count; k += LTD_THREADS) {
        const int      w = members[first + k], nc = dec[(size_t)w * 8 + 2];
        const int32_t *T = tab + (size_t)w * LT_TAB_INTS;
        const int      N = T[LT_N];
        const bool     ok = N <= LM_MAX_NODES;
        mword[k] = w;
        medges[k] = (uint8_t)(ok ? min(ltd_edges(N, (uint32_t)T[LT_S0], (uint32_t)T[LT_S1]), LTD_MAX_EDGES) : 255);
        mseed[k] = (uint8_t)(ok && nc >= 1 && nc <= LTD_MAX_LEN ? nc : 0);
    }
    if (tid < LTD_MAX_SEEDS) {
#pragma unroll
        for (int v = 0; v < LTD_WAVES; ++v) seed_a[v][tid] = 0;
    }
    __syncthreads();
    // the seeds: the first 32 usable slots with a string of 1 .. 32 labels, and the usable slots in order, by wave 0
    if (wave == 0) {
        int ns = 0, nu = 0;
        for (int base = 0; base < count; base += 64) {
            const int      k = base + lane;
            const bool     u = k < count && medges[k] != 255, q = u && mseed[k] > 0;
            const uint64_t um = __ballot(u), qm = __ballot(q), below = (1ull << lane) - 1ull;
            const int      ur = nu + __popcll(um & below), qr = ns + __popcll(qm & below);
            if (u) ulist[ur] = (uint16_t)k;
            if (q && qr < LTD_MAX_SEEDS) seed_slot[qr] = (int16_t)k;
            nu += __popcll(um); ns += __popcll(qm);
        }
        if (lane == 0) { wcount[0] = min(ns, LTD_MAX_SEEDS); wcount[1] = nu; }
    }
    if (tid == 64) {          // ... and whether the usable members' rows fit the pool, with their places, by one thread of wave 1
        int at = 0, fits = 1;
        for (int k = 0; k < count; ++k) {
            const int e = (int)medges[k];
            if (e == 255) continue;
            if (at + e > LTD_RES_EDGES) { fits = 0; break; }
            roff[k] = (uint16_t)at;
            at += e;
        }
        wcount[2] = fits;
    }
    __syncthreads();
    const int  n_seeds = wcount[0], used = wcount[1];
    const bool resident = wcount[2] != 0;          // (uniform)
    int32_t   *o = out + (size_t)t_ * 8;
    if (n_seeds == 0) {          // (uniform) not decoded
        if (tid == 0) { o[0] = -1; o[1] = -1; o[2] = 0; o[3] = 0; o[4] = 0; o[5] = used; o[6] = -1; o[7] = -1; }
        if (tid < LTD_MAX_LEN) chars[(size_t)t_ * LTD_MAX_LEN + tid] = 0xFF;
        return;
    }
    LtdMeta &Mw = meta[wave];
    if (resident)          // the rows of every usable member into the pool, a wave a member
        for (int p = wave; p < used; p += LTD_WAVES) {
            const int      k = (int)ulist[p];
            const int32_t *T = tab + (size_t)mword[k] * LT_TAB_INTS;
            wd_wave_sync();          // (the edge list of the member before is read)
            ltd_meta(Mw, T, lane);
            wd_wave_sync();
            ltd_stage(pool + (int)roff[k] * WD_ALPHABET, Mw, T, run_costs, piece_costs, lane, 64);
        }
    for (int e = tid; e < n_seeds * LTD_MAX_LEN; e += LTD_THREADS) {
        const int sd = e >> 5, pos = e & 31, k = seed_slot[sd];
        seeds[sd][pos] = pos < (int)mseed[k] ? dchars[(size_t)mword[k] * 64 + pos] : (uint8_t)0;
    }
    __syncthreads();
    if (tid < n_seeds) {
        const uint8_t *sv = seeds[tid];
        const int      l = (int)mseed[seed_slot[tid]];
        int32_t        c = (int32_t)Bs[WD_E * WD_ROW + sv[0]] + (int32_t)Bs[sv[l - 1] * WD_ROW + WD_E];
        for (int j = 0; j + 1 < l; ++j) c += (int32_t)Bs[sv[j] * WD_ROW + sv[j + 1]];
        seed_lm[tid] = c;
    }
    // J of every seed: a wave a member, its own edge list and (where the rows are not resident) staging buffer
    uint8_t *mine = pool + wave * LTD_SLOT;
    for (int p = wave; p < used; p += LTD_WAVES) {
        const int      k = (int)ulist[p];
        const int32_t *T = tab + (size_t)mword[k] * LT_TAB_INTS;
        wd_wave_sync();          // (the edge list and the rows of the member before are read)
        ltd_meta(Mw, T, lane);
        wd_wave_sync();
        const uint8_t *R = mine;
        if (resident) R = pool + (int)roff[k] * WD_ALPHABET;
        else {
            ltd_stage(mine, Mw, T, run_costs, piece_costs, lane, 64);
            wd_wave_sync();
        }
        for (int sd = 0; sd < n_seeds; ++sd) {
            const int c = ltd_forward<false>(R, Mw, seeds[sd], (int)mseed[seed_slot[sd]], ins, del, split, nullptr, lane);
            if (lane == 0) seed_a[wave][sd] += c;
        }
    }
    __syncthreads();
    if (wave == 0) {
        uint64_t key = LTD_NO_KEY;
        if (lane < n_seeds) {
            int32_t J = seed_lm[lane];
#pragma unroll
            for (int v = 0; v < LTD_WAVES; ++v) J += seed_a[v][lane];
            key = (uint64_t)(uint32_t)J << 8 | (uint32_t)lane;
        }
        key = ltd_wave_min(key);
        if (lane == 0) wk[0] = key;
    }
    __syncthreads();
    const int seed = (int)(wk[0] & 255u);
    int32_t   J = (int32_t)(wk[0] >> 8), lmS = seed_lm[seed];
    int       l = (int)mseed[seed_slot[seed]];
    const int32_t seed_cost = J, seed_member = mword[seed_slot[seed]];
    if (tid < LTD_MAX_LEN) str[tid] = seeds[seed][tid];
    __syncthreads();
    int       n_edits = 0, converged = 0;
    const int half = wave >> 1;          // the member of a pair whose tables this wave builds
    for (int round = 1; round <= rounds; ++round) {
        // which of the thread's neighbours exist at this length
        uint32_t live = 0;
#pragma unroll
        for (int q = 0; q < LTD_PER_THREAD; ++q) {
            const int x = tid + q * LTD_THREADS;
            bool      ok = false;
            if (x < LTD_DEL_AT) ok = x < l * WD_ALPHABET;
            else if (x < LTD_INS_AT) ok = l > 1 && x - LTD_DEL_AT < l;
            else if (x < LTD_NEIGHBOURS) ok = l < LTD_MAX_LEN && x - LTD_INS_AT < (l + 1) * WD_ALPHABET;
            live |= ok ? 1u << q : 0u;
            acc[q][tid] = 0;
        }
        for (int p = 0; p < used; p += 2) {          // two members at a time
            const int  n_here = min(2, used - p);
            const bool mineb = half < n_here;          // (uniform in the wave)
            __syncthreads();          // (the edge lists, rows and tables of the pair before are read)
            if (mineb && (wave & 1) == 0) ltd_meta(meta[half], tab + (size_t)mword[ulist[p + half]] * LT_TAB_INTS, lane);
            __syncthreads();
            const uint8_t *rows0 = pool, *rows1 = pool + LTD_SLOT;
            if (resident) {
                rows0 = pool + (int)roff[ulist[p]] * WD_ALPHABET;
                if (n_here > 1) rows1 = pool + (int)roff[ulist[p + 1]] * WD_ALPHABET;
            } else {
                ltd_stage(pool, meta[0], tab + (size_t)mword[ulist[p]] * LT_TAB_INTS, run_costs, piece_costs, tid, LTD_THREADS);
                if (n_here > 1) ltd_stage(pool + LTD_SLOT, meta[1], tab + (size_t)mword[ulist[p + 1]] * LT_TAB_INTS, run_costs, piece_costs, tid, LTD_THREADS);
                __syncthreads();
            }
            if (mineb) {
                const uint8_t *R = half ? rows1 : rows0;
                if ((wave & 1) == 0) ltd_forward<true>(R, meta[half], str, l, ins, del, split, F[half], lane);
                else ltd_backward(R, meta[half], str, l, ins, del, split, G[half], lane);
            }
            __syncthreads();
            for (int h = 0; h < n_here; ++h) {
                const uint8_t *R = h ? rows1 : rows0;
                for (uint32_t todo = live; todo; todo &= todo - 1u) {
                    const int q = __ffs((int)todo) - 1;
                    int       j, a, gg;
                    ltd_neighbour(tid + q * LTD_THREADS, j, a, gg);
                    acc[q][tid] += ltd_joined(F[h] + j * LTD_TS, G[h] + gg * LTD_TS, R, meta[h], a, ins, split);
                }
            }
        }
        uint64_t key = LTD_NO_KEY;
        for (uint32_t todo = live; todo; todo &= todo - 1u) {
            const int q = __ffs((int)todo) - 1;
            int       j, a, gg;
            ltd_neighbour(tid + q * LTD_THREADS, j, a, gg);
            const int pc = j > 0 ? (int)str[j - 1] : WD_E;
            int32_t   lm = lmS;
            if (gg == j) {          // INS
                const int nx = j < l ? (int)str[j] : WD_E;
                lm += (int32_t)Bs[pc * WD_ROW + a] + (int32_t)Bs[a * WD_ROW + nx] - (int32_t)Bs[pc * WD_ROW + nx];
            } else {
                const int old = (int)str[j], nx = j + 1 < l ? (int)str[j + 1] : WD_E;
                lm -= (int32_t)Bs[pc * WD_ROW + old] + (int32_t)Bs[old * WD_ROW + nx];
                lm += a >= 0 ? (int32_t)Bs[pc * WD_ROW + a] + (int32_t)Bs[a * WD_ROW + nx] : (int32_t)Bs[pc * WD_ROW + nx];
            }
            const uint64_t kq = (uint64_t)(uint32_t)(acc[q][tid] + lm) << 27 | (uint64_t)(uint32_t)(tid + q * LTD_THREADS) << 14 | (uint32_t)lm;
            key = kq < key ? kq : key;
        }
        key = ltd_wave_min(key);
        if (lane == 0) wk[wave] = key;
        __syncthreads();
        key = wk[0];
#pragma unroll
        for (int v = 1; v < LTD_WAVES; ++v) key = wk[v] < key ? wk[v] : key;
        const int32_t Jb = (int32_t)(key >> 27);
        if (key == LTD_NO_KEY || Jb >= J) { converged = 1; break; }          // (uniform)
        const int x = (int)(key >> 14 & 8191u);
        int       nl = l;
        if (x < LTD_DEL_AT) {
            if (tid == 0) str[x / WD_ALPHABET] = (uint8_t)(x % WD_ALPHABET);
        } else if (x < LTD_INS_AT) {
            if (tid == 0)
                for (int q = x - LTD_DEL_AT; q + 1 < l; ++q) str[q] = str[q + 1];
            nl = l - 1;
        } else {
            const int y = x - LTD_INS_AT, j = y / WD_ALPHABET;
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
    if (tid == 0) { o[0] = J; o[1] = seed_cost; o[2] = l; o[3] = n_edits; o[4] = converged; o[5] = used; o[6] = seed_member; o[7] = lmS; }
    if (tid < LTD_MAX_LEN) chars[(size_t)t_ * LTD_MAX_LEN + tid] = tid < l ? str[tid] : (uint8_t)0xFF;
}

// a wave per slot of the member array: for the string of the slot's track the member's own table and backtrack
__global__ void __launch_bounds__(64 * LTD_WAVES) k_lattice_track_decode_members(int ins, int del, int split, const str_er_run_split *__restrict__ splits,
                                                                                 const uint8_t *__restrict__ run_costs, const uint8_t *__restrict__ piece_costs,
                                                                                 const int32_t *__restrict__ first_run, const int32_t *__restrict__ n_of,
                                                                                 const int32_t *__restrict__ members, const int32_t *__restrict__ slot_track,
                                                                                 const int32_t *__restrict__ pslot, int n_members, const int32_t *__restrict__ out,
                                                                                 const uint8_t *__restrict__ chars, int32_t *__restrict__ mrec,
                                                                                 uint8_t *__restrict__ src, int32_t *__restrict__ parts)
{
    __shared__ LmWaveLds lds[LTD_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sl = (int)blockIdx.x * LTD_WAVES + wave;
    if (sl >= n_members) return;          // (no workgroup barrier below: a wave is on its own)
    const int t = __builtin_amdgcn_readfirstlane(slot_track[sl]);
    int32_t  *o = mrec + (size_t)sl * 6;
    if (t < 0) {          // (uniform) a slot of no track
        if (lane < 32) src[(size_t)sl * 32 + lane] = 0xFF;
        if (lane == 0) { o[0] = -1; o[1] = o[2] = o[3] = o[4] = 0; o[5] = -1; }
        return;
    }
    const int      w = __builtin_amdgcn_readfirstlane(members[sl]);
    const int      first = __builtin_amdgcn_readfirstlane(first_run[w]), m = max(0, __builtin_amdgcn_readfirstlane(n_of[w]));
    const size_t   base = (size_t)__builtin_amdgcn_readfirstlane(pslot[sl]);
    const int      l = min(max(__builtin_amdgcn_readfirstlane(out[(size_t)t * 8 + 2]), 0), LTD_MAX_LEN);
    const WmParams prm{ins, del, 0};
    LmWaveLds     &L = lds[wave];
    int            N = 0;
    lm_wave_nodes(L, splits, run_costs, piece_costs, first, m, split, lane, N);
    const bool run = l > 0 && N <= LM_MAX_NODES;          // (a decoded track's string has a label)
    lm_wave_labels(L, prm, split, run_costs, piece_costs, chars + (size_t)t * LTD_MAX_LEN, l, N, run, lane);
    lm_wave_sync();
    lm_wave_store(L, run ? l : 0, lane, src + (size_t)sl * 32, parts + 2 * base);          // (n_parts <= N: inside the slot's part slots)
    if (lane == 0) {
        o[0] = run ? L.T[N * LM_TROW + l] : -1;
        o[1] = 0; o[2] = L.rec[0]; o[3] = L.rec[1]; o[4] = L.rec[2]; o[5] = w;
    }
}

} // namespace

void launch_lattice_track_decode_tab(hipStream_t s, const uint8_t *bigram, int ins, int del, int rounds, int split, const str_er_run_split *splits, const uint8_t *run_costs,
                                     const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of, const void *dec, const uint8_t *dchars,
                                     const int32_t *track_first, const int32_t *track_count, const int32_t *members, const int32_t *slot_track, const int32_t *pslot,
                                     int n_members, int n_tracks, const int32_t *tab, void *out, uint8_t *chars, int32_t *mrec, uint8_t *src, int32_t *parts)
{
    if (n_tracks > 0)
        hipLaunchKernelGGL(k_lattice_track_decode, dim3((unsigned)n_tracks), dim3(LTD_THREADS), 0, s, bigram, ins, del, rounds, split, run_costs, piece_costs, tab,
                           static_cast<const int32_t *>(dec), dchars, track_first, track_count, members, static_cast<int32_t *>(out), chars);
    if (n_members > 0)
        hipLaunchKernelGGL(k_lattice_track_decode_members, dim3((unsigned)((n_members + LTD_WAVES - 1) / LTD_WAVES)), dim3(64 * LTD_WAVES), 0, s, ins, del, split, splits,
                           run_costs, piece_costs, first_run, n_of, members, slot_track, pslot, n_members, static_cast<const int32_t *>(out), chars, mrec, src, parts);
}

void launch_lattice_track_decode(hipStream_t s, const uint8_t *bigram, int ins, int del, int rounds, int split, const str_er_run_split *splits, const uint8_t *run_costs,
                                 const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of, int n_words, const void *dec, const uint8_t *dchars,
                                 const int32_t *track_first, const int32_t *track_count, const int32_t *members, const int32_t *slot_track, const int32_t *pslot,
                                 int n_members, int n_tracks, int32_t *tab, void *out, uint8_t *chars, int32_t *mrec, uint8_t *src, int32_t *parts)
{
    if (n_tracks > 0) launch_lattice_track_table(s, del, split, splits, first_run, n_of, n_words, tab);
    launch_lattice_track_decode_tab(s, bigram, ins, del, rounds, split, splits, run_costs, piece_costs, first_run, n_of, dec, dchars, track_first, track_count, members,
                                    slot_track, pslot, n_members, n_tracks, tab, out, chars, mrec, src, parts);
}

} // namespace str_er
