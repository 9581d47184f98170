// decode_pool_kernels.hip -- the decode pool on the device (gfx950): the store of the kept members' rows, from which k_track_decode
// (track_decode_kernels.hip) reads a slot as it reads the track of one call.  k_dpool_keep places the usable members of a call's
// tracks into their slots and evicts the oldest; k_dpool_join merges the kept lists of slots; k_dpool_plan ranks the keys of every slot
// asked for and writes the track tables of the read; k_dpool_records makes the records from what k_track_decode left.  Integers only,
// no atomics and no scratch; every loop is bounded (keep <= 1024 cells, at most 65536 members a track, n_srcs slots) and no workgroup
// waits for another: a workgroup owns the slot it writes (the slots of a call are distinct), so the pool holds the same bytes every
// run.  The rules are stated for the host in decode_pool_rules.h; the contract is at str_er_pool_decode in str_er.h.
//
// The placement (which cells stay, which cell an incoming member takes) is decode_pool_device.h, shared with the lattice decode pool.
#include <hip/hip_runtime.h>

#include "decode_pool_device.h"
#include "decode_pool_kernels.h"

namespace str_er {

namespace {

constexpr int DP_ALPHABET = 65, DP_MAX_ROWS = 32, DP_CHARS = 64, DP_DEC_INTS = 6;
constexpr int DP_CELL_CHUNKS = DP_CELL_ROW_BYTES / 16;
static_assert(DP_CELL_ROW_BYTES % 16 == 0, "cell layout");

// the decoder's record and labels of a member into a cell, by the lanes of a wave
__device__ __forceinline__ void dp_copy_strings(const DpPoolDev &pool, size_t cell, const int32_t *dec, const uint8_t *dchars, int lane)
{
    if (lane < DP_DEC_INTS) pool.dec[cell * DP_DEC_INTS + lane] = dec[lane];
    if (lane < DP_CHARS / 16) reinterpret_cast<uint4 *>(pool.dchars + cell * DP_CHARS)[lane] = reinterpret_cast<const uint4 *>(dchars)[lane];
}

// One workgroup per track of the call.
__global__ void __launch_bounds__(DP_THREADS) k_dpool_keep(DpPoolDev pool, uint32_t serial, const uint8_t *__restrict__ costs, const int32_t *__restrict__ first_run,
                                                           const int32_t *__restrict__ n_of, const int32_t *__restrict__ dec, const uint8_t *__restrict__ dchars,
                                                           const int32_t *__restrict__ track_first, const int32_t *__restrict__ track_count,
                                                           const int32_t *__restrict__ members, const int32_t *__restrict__ slots)
{
    __shared__ DpKeepLds L;
    const int    t = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int    first = track_first[t], count = track_count[t], slot = slots[t], keep = pool.keep;
    const size_t c0 = (size_t)slot * (size_t)keep;
    // the usable members of the call: at most 32 rows
    const int nin = dp_place_add(L, pool.key + c0, keep, first, count, members, [&](int w) { return n_of[w] <= DP_MAX_ROWS; }, tid);
    // a wave a survivor: its rows come from any multiple of 65 bytes, so they are read byte by byte; the cell takes 16-byte stores
    for (int i = wave; i < nin; i += DP_WAVES) {
        const int      idx = L.inc[i], w = members[idx], m = max(n_of[w], 0), n_bytes = m * DP_ALPHABET;
        const size_t   cell = c0 + (size_t)L.cell_of[i];
        const uint8_t *src = costs + (size_t)first_run[w] * DP_ALPHABET;
        uint4         *dst = reinterpret_cast<uint4 *>(pool.costs + cell * DP_CELL_ROW_BYTES);
        for (int ch = lane; ch * 16 < n_bytes; ch += 64) {
            uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const int e = ch * 16 + b;
                if (e < n_bytes) v[b >> 2] |= (uint32_t)src[e] << (8 * (b & 3));
            }
            dst[ch] = make_uint4(v[0], v[1], v[2], v[3]);
        }
        dp_copy_strings(pool, cell, dec + (size_t)w * DP_DEC_INTS, dchars + (size_t)w * DP_CHARS, lane);
        if (lane == 0) {
            pool.n_of[cell] = m;
            pool.key[cell] = (uint64_t)serial << 32 | (uint32_t)idx;
        }
    }
    if (tid == 0) pool.n_members[slot] += count;
}

// One workgroup: dst takes the srcs one at a time.
__global__ void __launch_bounds__(DP_THREADS) k_dpool_join(DpPoolDev pool, int dst, const int32_t *__restrict__ srcs, int n_srcs)
{
    __shared__ DpJoinLds L;
    const int    tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, keep = pool.keep;
    const size_t d0 = (size_t)dst * (size_t)keep;
    for (int c = tid; c < keep; c += DP_THREADS) L.dkey[c] = pool.key[d0 + c];
    int32_t joined = 0;          // (thread 0) the members of the srcs
    for (int k = 0; k < n_srcs; ++k) {
        const int    src = srcs[k];
        const size_t s0 = (size_t)src * (size_t)keep;
        const int    n_in = dp_place_join(L, pool.key + d0, pool.key + s0, keep, tid);
        // a wave a survivor, cell to cell in 16-byte pieces
        for (int i = wave; i < n_in; i += DP_WAVES) {
            const size_t from = s0 + (size_t)L.take[i], to = d0 + (size_t)L.cell_of[i];
            const int    m = pool.n_of[from], n_bytes = m * DP_ALPHABET;
            const uint4 *a = reinterpret_cast<const uint4 *>(pool.costs + from * DP_CELL_ROW_BYTES);
            uint4       *b = reinterpret_cast<uint4 *>(pool.costs + to * DP_CELL_ROW_BYTES);
            for (int ch = lane; ch < DP_CELL_CHUNKS && ch * 16 < n_bytes; ch += 64) b[ch] = a[ch];
            dp_copy_strings(pool, to, pool.dec + from * DP_DEC_INTS, pool.dchars + from * DP_CHARS, lane);
            if (lane == 0) {
                pool.n_of[to] = m;
                pool.key[to] = L.skey[L.take[i]];
                L.dkey[L.cell_of[i]] = L.skey[L.take[i]];
            }
        }
        for (int c = tid; c < keep; c += DP_THREADS) pool.key[s0 + c] = 0;
        if (tid == 0) { joined += pool.n_members[src]; pool.n_members[src] = 0; }
    }
    if (tid == 0) pool.n_members[dst] += joined;
}

// one workgroup per slot named: its cells empty, its count 0
__global__ void __launch_bounds__(DP_THREADS) k_dpool_clear(DpPoolDev pool, const int32_t *__restrict__ slots)
{
    const int    slot = slots[blockIdx.x], tid = (int)threadIdx.x;
    const size_t c0 = (size_t)slot * (size_t)pool.keep;
    for (int c = tid; c < pool.keep; c += DP_THREADS) pool.key[c0 + c] = 0;
    if (tid == 0) pool.n_members[slot] = 0;
}

// a thread a cell: empty, its rows at 32 * cell; the first cap threads the counts
__global__ void __launch_bounds__(DP_THREADS) k_dpool_reset(DpPoolDev pool, int n_cells)
{
    const int w = (int)blockIdx.x * DP_THREADS + (int)threadIdx.x;
    if (w < n_cells) { pool.key[w] = 0; pool.n_of[w] = 0; pool.first_run[w] = DP_MAX_ROWS * w; }
    if (w < pool.cap) pool.n_members[w] = 0;
}

// One workgroup per slot asked for: the age rank of a kept cell is the number of kept keys below its own.
__global__ void __launch_bounds__(DP_THREADS) k_dpool_plan(DpPoolDev pool, const int32_t *__restrict__ slots, int32_t *__restrict__ track_first,
                                                           int32_t *__restrict__ track_count, int32_t *__restrict__ members, int32_t *__restrict__ rank_of,
                                                           int32_t *__restrict__ member_cost)
{
    __shared__ uint64_t key[DP_MAX_KEEP];
    __shared__ int      wsum[DP_WAVES];
    const int    i = (int)blockIdx.x, tid = (int)threadIdx.x, keep = pool.keep, slot = slots[i];
    const size_t c0 = (size_t)slot * (size_t)keep, at = (size_t)i * (size_t)keep;
    for (int c = tid; c < keep; c += DP_THREADS) key[c] = pool.key[c0 + c];
    __syncthreads();
    int n = 0;
    for (int c = tid; c < keep; c += DP_THREADS) {
        const uint64_t mine = key[c];
        int            rank = -1;
        if (mine != 0) {
            rank = 0;
            for (int k = 0; k < keep; ++k) rank += key[k] != 0 && key[k] < mine ? 1 : 0;
            members[at + rank] = (int32_t)(c0 + c);
            ++n;
        }
        rank_of[at + c] = rank;
        member_cost[at + c] = -1;
    }
    int n_kept;
    dp_scan(n, wsum, tid, n_kept);
    if (tid == 0) { track_first[i] = (int32_t)at; track_count[i] = n_kept; }
}

// a thread a slot asked for
__global__ void __launch_bounds__(DP_THREADS) k_dpool_records(DpPoolDev pool, const int32_t *__restrict__ slots, int n, const int32_t *__restrict__ rec,
                                                              const int32_t *__restrict__ track_count, const int32_t *__restrict__ rank_of, int32_t *__restrict__ out)
{
    const int i = (int)blockIdx.x * DP_THREADS + (int)threadIdx.x;
    if (i >= n) return;
    const int      slot = slots[i];
    const int32_t *r = rec + (size_t)i * 8;
    int32_t       *o = out + (size_t)i * 10;
#pragma unroll
    for (int f = 0; f < 8; ++f) o[f] = r[f];
    if (r[6] >= 0) o[6] = rank_of[(size_t)i * (size_t)pool.keep + (size_t)(r[6] - slot * pool.keep)];
    o[8] = pool.n_members[slot];
    o[9] = track_count[i];
}

} // namespace

void launch_dpool_reset(hipStream_t s, const DpPoolDev &pool)
{
    const int n_cells = pool.cap * pool.keep;
    hipLaunchKernelGGL(k_dpool_reset, dim3((unsigned)((n_cells + DP_THREADS - 1) / DP_THREADS)), dim3(DP_THREADS), 0, s, pool, n_cells);
}

void launch_dpool_keep(hipStream_t s, const DpPoolDev &pool, uint32_t serial, const uint8_t *costs, const int32_t *first_run, const int32_t *n_of, const void *dec,
                       const uint8_t *dchars, const int32_t *track_first, const int32_t *track_count, const int32_t *members, const int32_t *slots, int n_tracks)
{
    if (n_tracks <= 0) return;
    hipLaunchKernelGGL(k_dpool_keep, dim3((unsigned)n_tracks), dim3(DP_THREADS), 0, s, pool, serial, costs, first_run, n_of, static_cast<const int32_t *>(dec), dchars,
                       track_first, track_count, members, slots);
}

void launch_dpool_join(hipStream_t s, const DpPoolDev &pool, int dst, const int32_t *srcs, int n_srcs)
{
    if (n_srcs <= 0) return;
    hipLaunchKernelGGL(k_dpool_join, dim3(1), dim3(DP_THREADS), 0, s, pool, dst, srcs, n_srcs);
}

void launch_dpool_clear(hipStream_t s, const DpPoolDev &pool, const int32_t *slots, int n)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_dpool_clear, dim3((unsigned)n), dim3(DP_THREADS), 0, s, pool, slots);
}

void launch_dpool_plan(hipStream_t s, const DpPoolDev &pool, const int32_t *slots, int n, int32_t *track_first, int32_t *track_count, int32_t *members, int32_t *rank_of,
                       int32_t *member_cost)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_dpool_plan, dim3((unsigned)n), dim3(DP_THREADS), 0, s, pool, slots, track_first, track_count, members, rank_of, member_cost);
}

void launch_dpool_records(hipStream_t s, const DpPoolDev &pool, const int32_t *slots, int n, const int32_t *rec, const int32_t *track_count, const int32_t *rank_of,
                          int32_t *out)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_dpool_records, dim3((unsigned)((n + DP_THREADS - 1) / DP_THREADS)), dim3(DP_THREADS), 0, s, pool, slots, n, rec, track_count, rank_of, out);
}

} // namespace str_er
