// lattice_decode_pool_kernels.hip -- the lattice decode pool on the device (gfx950): the store of the kept members' runs, pieces and
// split records, from which k_lattice_track_decode and k_lattice_track_decode_members (lattice_track_decode_kernels.hip) read a slot as
// they read the track of one call.  k_ldpool_keep places the usable members of a call's tracks into their slots, evicts the oldest and
// gathers a member's evidence into its cell; k_ldpool_join merges the kept lists of slots; k_dpool_plan (decode_pool_kernels.hip) ranks
// the keys of every slot asked for; k_ldpool_tracks completes the track tables of the read and makes the structure row of every cell
// it names; k_ldpool_records turns cells into age ranks in what the decode left.  Integers only, no atomics and no scratch; every loop
// is bounded (keep <= 1024 cells, at most 65536 members a track, 32 runs, 72 pieces, n_srcs slots) and no workgroup waits for another: a
// workgroup owns the slot it writes (the slots of a call are distinct), so the pool holds the same bytes every run.  The rules are
// stated for the host in lattice_decode_pool_rules.h; the placement is decode_pool_device.h, shared with the decode pool.
#include <hip/hip_runtime.h>

#include "decode_pool_device.h"
#include "lattice_decode_pool_kernels.h"
#include "lattice_track_device.h"

namespace str_er {

namespace {

constexpr int LDP_ALPHABET = 65, LDP_CHARS = 64, LDP_DEC_INTS = 8, LDP_PARTS = 32;      // (part slots of a member of a read: N <= 32)
constexpr int LDP_PIECES_USED = 72;
// (lt_table_row keeps a piece's row as index | LM_PIECE and the track decode masks the flag off: every piece row of the store lies below it)
static_assert((long long)LDP_MAX_CELLS * LDP_CELL_PIECES <= (long long)LM_PIECE, "the store's piece rows and the flag of the structure table");
static_assert(LDP_CELL_RUN_BYTES % 16 == 0 && LDP_CELL_PIECE_BYTES % 16 == 0 && LDP_CELL_RUNS == LM_MAX_NODES && sizeof(str_er_run_split) == 32, "cell layout");

// the pieces of a run of A atoms (1 .. 4): 0, 2, 5 or 9
__device__ __forceinline__ int ldp_pieces(int A) { return A * (A + 1) / 2 - 1; }

// whether the call's word (first, m) can be kept: N <= 32, which implies at most 32 runs
__device__ __forceinline__ bool ldp_usable(const str_er_run_split *__restrict__ splits, int first, int m)
{
    if (m > LDP_CELL_RUNS) return false;
    int N = 0;
    for (int t = 0; t < m; ++t) N += lm_atoms(splits, first + t);
    return N <= LM_MAX_NODES;
}

// n_bytes bytes from src (any alignment, read byte by byte) to dst (16-byte stores; the last one is padded with zeroes), by a wave
__device__ __forceinline__ void ldp_gather(uint4 *dst, const uint8_t *__restrict__ src, int n_bytes, int lane)
{
    for (int ch = lane; ch * 16 < n_bytes; ch += 64) {
        uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const int e = ch * 16 + b;
            if (e < n_bytes) v[b >> 2] |= (uint32_t)src[e] << (8 * (b & 3));
        }
        dst[ch] = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

// the lattice decoder's record and labels of a member into a cell, by the lanes of a wave
__device__ __forceinline__ void ldp_copy_strings(const LdpPoolDev &pool, size_t cell, const int32_t *dec, const uint8_t *dchars, int lane)
{
    if (lane < LDP_DEC_INTS) pool.dec[cell * LDP_DEC_INTS + lane] = dec[lane];
    if (lane < LDP_CHARS / 16) reinterpret_cast<uint4 *>(pool.dchars + cell * LDP_CHARS)[lane] = reinterpret_cast<const uint4 *>(dchars)[lane];
}

// the exclusive prefix sum of v over the lanes of a wave
__device__ __forceinline__ int ldp_wave_scan(int v, int lane)
{
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    return inc - v;
}

// One workgroup per track of the call.
__global__ void __launch_bounds__(DP_THREADS) k_ldpool_keep(LdpPoolDev pool, uint32_t serial, const str_er_run_split *__restrict__ splits,
                                                            const uint8_t *__restrict__ run_costs, const uint8_t *__restrict__ piece_costs,
                                                            const int32_t *__restrict__ first_run, const int32_t *__restrict__ n_of, const int32_t *__restrict__ dec,
                                                            const uint8_t *__restrict__ dchars, const int32_t *__restrict__ track_first,
                                                            const int32_t *__restrict__ track_count, const int32_t *__restrict__ members,
                                                            const int32_t *__restrict__ slots)
{
    __shared__ DpKeepLds L;
    __shared__ int32_t   pfrom[DP_WAVES][LDP_CELL_PIECES];          // per wave: the call's piece row of every piece row of the cell
    const int    t = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int    first = track_first[t], count = track_count[t], slot = slots[t], keep = pool.keep;
    const size_t c0 = (size_t)slot * (size_t)keep;
    const int    nin = dp_place_add(L, pool.key + c0, keep, first, count, members, [&](int w) { return ldp_usable(splits, first_run[w], n_of[w]); }, tid);
    // a wave a survivor: its rows come from any multiple of 65 bytes, so they are read byte by byte; the cell takes 16-byte stores
    for (int i = wave; i < nin; i += DP_WAVES) {
        const int    idx = L.inc[i], w = members[idx], m = min(max(n_of[w], 0), LDP_CELL_RUNS), f = first_run[w];
        const size_t cell = c0 + (size_t)L.cell_of[i];
        ldp_gather(reinterpret_cast<uint4 *>(pool.run_rows + cell * LDP_CELL_RUN_BYTES), run_costs + (size_t)f * LDP_ALPHABET, m * LDP_ALPHABET, lane);
        // lane t takes the run t: where its pieces go (back to back in run order), and its record with first_piece rebased into the cell
        uint4 lo = make_uint4(0, 0, 0, 0), hi = make_uint4(0, 0, 0, 0);
        int   np = 0, fp = 0;
        if (lane < m) {
            const uint4 *S = reinterpret_cast<const uint4 *>(splits + f + lane);
            lo = S[0]; hi = S[1];
            np = ldp_pieces(min(max((int)lo.x, 0), 3) + 1);          // (from n_cuts: N <= 32 then bounds the sum by 72)
            fp = (int)hi.y;
        }
        const int base = ldp_wave_scan(np, lane);
        int       total = __shfl(base + np, 63, 64);
        total = min(total, LDP_PIECES_USED);
        if (lane < m) hi.y = (uint32_t)((int)cell * LDP_CELL_PIECES + base);
        lm_wave_sync();          // (the list of the member before is read)
        for (int k = 0; k < np; ++k)
            if (base + k < LDP_CELL_PIECES) pfrom[wave][base + k] = fp + k;
        lm_wave_sync();
        {
            uint4    *dst = reinterpret_cast<uint4 *>(pool.piece_rows + cell * LDP_CELL_PIECE_BYTES);
            const int n_bytes = total * LDP_ALPHABET;
            for (int ch = lane; ch * 16 < n_bytes; ch += 64) {
                uint32_t v[4] = {0, 0, 0, 0};
                // (the chunk's first byte is byte a of the cell's piece row q; a chunk of 16 bytes meets at most two rows)
                int            q = ch * 16 / LDP_ALPHABET, a = ch * 16 - q * LDP_ALPHABET;
                const uint8_t *row = piece_costs + (size_t)pfrom[wave][q] * LDP_ALPHABET;
#pragma unroll
                for (int b = 0; b < 16; ++b) {
                    if (ch * 16 + b < n_bytes) {
                        v[b >> 2] |= (uint32_t)row[a] << (8 * (b & 3));
                        if (++a == LDP_ALPHABET && ch * 16 + b + 1 < n_bytes) { a = 0; row = piece_costs + (size_t)pfrom[wave][++q] * LDP_ALPHABET; }
                    }
                }
                dst[ch] = make_uint4(v[0], v[1], v[2], v[3]);
            }
        }
        if (lane < LDP_CELL_RUNS) {          // (the records past the member's runs are zeroes)
            uint4 *R = reinterpret_cast<uint4 *>(pool.splits + cell * LDP_CELL_RUNS + lane);
            R[0] = lo; R[1] = hi;
        }
        ldp_copy_strings(pool, cell, dec + (size_t)w * LDP_DEC_INTS, dchars + (size_t)w * LDP_CHARS, lane);
        if (lane == 0) {
            pool.n_of[cell] = m;
            pool.key[cell] = (uint64_t)serial << 32 | (uint32_t)idx;
        }
    }
    if (tid == 0) pool.n_members[slot] += count;
}

// One workgroup: dst takes the srcs one at a time.
__global__ void __launch_bounds__(DP_THREADS) k_ldpool_join(LdpPoolDev pool, int dst, const int32_t *__restrict__ srcs, int n_srcs)
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
            const int    m = min(max(pool.n_of[from], 0), LDP_CELL_RUNS);
            // lane t: the record of the run t, moved with the cell; the piece rows in use end where the last run's pieces end
            uint4 lo = make_uint4(0, 0, 0, 0), hi = make_uint4(0, 0, 0, 0);
            int   end = 0;
            if (lane < m) {
                const uint4 *S = reinterpret_cast<const uint4 *>(pool.splits + from * LDP_CELL_RUNS + lane);
                lo = S[0]; hi = S[1];
                const int local = (int)hi.y - (int)from * LDP_CELL_PIECES;
                end = local + ldp_pieces(min(max((int)lo.x, 0), 3) + 1);
                hi.y = (uint32_t)((int)to * LDP_CELL_PIECES + local);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) end = max(end, __shfl_xor(end, off, 64));
            end = min(max(end, 0), LDP_CELL_PIECES);
            const int    run_bytes = m * LDP_ALPHABET, piece_bytes = end * LDP_ALPHABET;
            const uint4 *a = reinterpret_cast<const uint4 *>(pool.run_rows + from * LDP_CELL_RUN_BYTES);
            uint4       *b = reinterpret_cast<uint4 *>(pool.run_rows + to * LDP_CELL_RUN_BYTES);
            for (int ch = lane; ch < LDP_CELL_RUN_BYTES / 16 && ch * 16 < run_bytes; ch += 64) b[ch] = a[ch];
            a = reinterpret_cast<const uint4 *>(pool.piece_rows + from * LDP_CELL_PIECE_BYTES);
            b = reinterpret_cast<uint4 *>(pool.piece_rows + to * LDP_CELL_PIECE_BYTES);
            for (int ch = lane; ch < LDP_CELL_PIECE_BYTES / 16 && ch * 16 < piece_bytes; ch += 64) b[ch] = a[ch];
            if (lane < LDP_CELL_RUNS) {
                uint4 *R = reinterpret_cast<uint4 *>(pool.splits + to * LDP_CELL_RUNS + lane);
                R[0] = lo; R[1] = hi;
            }
            ldp_copy_strings(pool, to, pool.dec + from * LDP_DEC_INTS, pool.dchars + from * LDP_CHARS, lane);
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

// a thread a cell: empty, its runs at 32 * cell; the first cap threads the counts
__global__ void __launch_bounds__(DP_THREADS) k_ldpool_reset(LdpPoolDev pool, int n_cells)
{
    const int w = (int)blockIdx.x * DP_THREADS + (int)threadIdx.x;
    if (w < n_cells) { pool.key[w] = 0; pool.n_of[w] = 0; pool.first_run[w] = LDP_CELL_RUNS * w; }
    if (w < pool.cap) pool.n_members[w] = 0;
}

// a thread a slot of the read's member array
__global__ void __launch_bounds__(DP_THREADS) k_ldpool_tracks(LdpPoolDev pool, int del, int split, int n_slots, const int32_t *__restrict__ lead,
                                                              const int32_t *__restrict__ track_count,
                                                              const int32_t *__restrict__ members, int32_t *__restrict__ slot_track, int32_t *__restrict__ pslot)
{
    const int sl = (int)blockIdx.x * DP_THREADS + (int)threadIdx.x;
    if (sl >= n_slots) return;
    const int  i = sl / pool.keep, r = sl - i * pool.keep;
    const bool kept = r < track_count[i];
    slot_track[sl] = kept ? i : -1;
    pslot[sl] = sl * LDP_PARTS;
    if (!kept || !lead[i]) return;          // (a slot named again in one read: the first request makes its cells' rows)
    const int cell = members[sl];
    lt_table_row(pool.tab + (size_t)cell * LT_TAB_INTS, del, split, pool.splits, LDP_CELL_RUNS * cell, pool.n_of[cell]);
}

// a thread a slot of the read's member array; the first of a request also makes its record
__global__ void __launch_bounds__(DP_THREADS) k_ldpool_records(LdpPoolDev pool, const int32_t *__restrict__ slots, int n_slots, const int32_t *__restrict__ rec,
                                                               const int32_t *__restrict__ track_count, const int32_t *__restrict__ members,
                                                               const int32_t *__restrict__ rank_of, const int32_t *__restrict__ pslot, int32_t *__restrict__ out,
                                                               int32_t *__restrict__ mrec, int32_t *__restrict__ parts, int32_t *__restrict__ member_cost)
{
    const int sl = (int)blockIdx.x * DP_THREADS + (int)threadIdx.x;
    if (sl >= n_slots) return;
    const int keep = pool.keep, i = sl / keep, r = sl - i * keep, slot = slots[i];
    if (r == 0) {
        const int32_t *q = rec + (size_t)i * 8;
        int32_t       *o = out + (size_t)i * 10;
#pragma unroll
        for (int f = 0; f < 8; ++f) o[f] = q[f];
        if (q[6] >= 0) o[6] = rank_of[(size_t)i * (size_t)keep + (size_t)(q[6] - slot * keep)];
        o[8] = pool.n_members[slot];
        o[9] = track_count[i];
    }
    if (r >= track_count[i]) return;
    const int cell = members[sl];
    int32_t  *m = mrec + (size_t)sl * 6;
    const int np = min(max(m[2], 0), LDP_PARTS), d_run = LDP_CELL_RUNS * (r - cell), d_piece = LDP_CELL_PIECES * (r - cell);
    int32_t  *p = parts + 2 * (size_t)pslot[sl];
    for (int k = 0; k < np; ++k) {
        p[2 * k] += d_run;
        if (p[2 * k + 1] >= 0) p[2 * k + 1] += d_piece;
    }
    m[5] = r;
    member_cost[sl] = m[0];
}

} // namespace

void launch_ldpool_reset(hipStream_t s, const LdpPoolDev &pool)
{
    const int n_cells = pool.cap * pool.keep;
    hipLaunchKernelGGL(k_ldpool_reset, dim3((unsigned)((n_cells + DP_THREADS - 1) / DP_THREADS)), dim3(DP_THREADS), 0, s, pool, n_cells);
}

void launch_ldpool_keep(hipStream_t s, const LdpPoolDev &pool, uint32_t serial, const str_er_run_split *splits, const uint8_t *run_costs, const uint8_t *piece_costs,
                        const int32_t *first_run, const int32_t *n_of, const void *dec, const uint8_t *dchars, const int32_t *track_first, const int32_t *track_count,
                        const int32_t *members, const int32_t *slots, int n_tracks)
{
    if (n_tracks <= 0) return;
    hipLaunchKernelGGL(k_ldpool_keep, dim3((unsigned)n_tracks), dim3(DP_THREADS), 0, s, pool, serial, splits, run_costs, piece_costs, first_run, n_of,
                       static_cast<const int32_t *>(dec), dchars, track_first, track_count, members, slots);
}

void launch_ldpool_join(hipStream_t s, const LdpPoolDev &pool, int dst, const int32_t *srcs, int n_srcs)
{
    if (n_srcs <= 0) return;
    hipLaunchKernelGGL(k_ldpool_join, dim3(1), dim3(DP_THREADS), 0, s, pool, dst, srcs, n_srcs);
}

void launch_ldpool_tracks(hipStream_t s, const LdpPoolDev &pool, int del, int split, int n, const int32_t *lead, const int32_t *track_count, const int32_t *members,
                          int32_t *slot_track,                          int32_t *pslot)
{
    if (n <= 0) return;
    const int n_slots = n * pool.keep;
    hipLaunchKernelGGL(k_ldpool_tracks, dim3((unsigned)((n_slots + DP_THREADS - 1) / DP_THREADS)), dim3(DP_THREADS), 0, s, pool, del, split, n_slots, lead, track_count,
                       members, slot_track, pslot);
}

void launch_ldpool_records(hipStream_t s, const LdpPoolDev &pool, const int32_t *slots, int n, const int32_t *rec, const int32_t *track_count, const int32_t *members,
                           const int32_t *rank_of, const int32_t *pslot, int32_t *out, int32_t *mrec, int32_t *parts, int32_t *member_cost)
{
    if (n <= 0) return;
    const int n_slots = n * pool.keep;
    hipLaunchKernelGGL(k_ldpool_records, dim3((unsigned)((n_slots + DP_THREADS - 1) / DP_THREADS)), dim3(DP_THREADS), 0, s, pool, slots, n_slots, rec, track_count, members,
                       rank_of, pslot, out, mrec, parts, member_cost);
}

} // namespace str_er
