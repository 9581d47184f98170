// decode_pool_device.h -- INTERNAL, device code: the placement that the decode pool (decode_pool_kernels.hip) and the lattice decode
// pool (lattice_decode_pool_kernels.hip) share.  Both keep, per slot, the `keep` largest keys of everything added or joined; they differ
// in what a cell holds, that is in the copy behind the placement.  One 256-thread workgroup owns the slot it writes.
//
// Placement, the same for an addition and a join: the survivors are the `keep` largest keys of old and incoming together.  A surviving
// old cell stays where it is; the i-th freed or empty cell, ascending, takes the i-th incoming survivor, ascending by key (a prefix sum
// over the cells).  Keys are ranked by counting in LDS: at most 1024 x 1024 comparisons a workgroup.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace str_er {

namespace {

constexpr int DP_THREADS = 256, DP_WAVES = DP_THREADS / 64;
constexpr int DP_MAX_KEEP = 1024, DP_PER_THREAD = DP_MAX_KEEP / DP_THREADS;      // a thread takes up to four neighbouring cells
static_assert(DP_PER_THREAD == 4, "cell layout");

// the exclusive prefix sum of v over the workgroup's threads and its total; called by every thread (wsum: DP_WAVES ints of LDS)
__device__ __forceinline__ int dp_scan(int v, int *wsum, int tid, int &total)
{
    const int lane = tid & 63, wave = tid >> 6;
    int       inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    __syncthreads();          // (the sums of the scan before are read)
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < DP_WAVES; ++w) {
        if (w < wave) base += wsum[w];
        total += wsum[w];
    }
    return base + inc - v;
}

// how many of the n keys at k (LDS) are larger than key
__device__ __forceinline__ int dp_larger(const uint64_t *k, int n, uint64_t key)
{
    int g = 0;
    for (int i = 0; i < n; ++i) g += k[i] > key ? 1 : 0;
    return g;
}

// the LDS of an addition's placement
struct DpKeepLds {
    uint64_t okey[DP_MAX_KEEP];
    int32_t  inc[DP_MAX_KEEP];            // the i-th incoming survivor, ascending: its index in the member array
    int32_t  cell_of[DP_MAX_KEEP];        // ... and the cell it takes
    int      wsum[DP_WAVES];
};

// The placement of an addition, by the whole workgroup: the track's members are members[first .. first + count), usable(w) says whether
// the call's word w can be kept, key [keep] are the keys of the slot's cells in global memory.  Returns the number of incoming
// survivors; L.inc and L.cell_of hold them, and the evicted cells nothing takes are emptied.  It ends on a barrier.
//   The keys of a call ascend with the index and are all larger than the slot's, so the newest min(U, keep) of its U usable members
// survive and nothing else of the call is ever written.
template <class Usable>
__device__ __forceinline__ int dp_place_add(DpKeepLds &L, uint64_t *key, int keep, int first, int count, const int32_t *__restrict__ members, Usable usable, int tid)
{
    for (int c = tid; c < keep; c += DP_THREADS) L.okey[c] = key[c];
    int u = 0;
    for (int j = tid; j < count; j += DP_THREADS) u += usable(members[first + j]) ? 1 : 0;
    int U;
    dp_scan(u, L.wsum, tid, U);          // (okey is written behind its barriers)
    const int nin = min(U, keep), skip = U - nin;
    int       base = 0;
    for (int j0 = 0; j0 < count; j0 += DP_THREADS) {          // (at most 256 rounds: a track has at most 65536 members)
        const int  j = j0 + tid;
        const bool q = j < count && usable(members[first + j]);
        int        total;
        const int  r = base + dp_scan(q ? 1 : 0, L.wsum, tid, total);
        if (q && r >= skip) L.inc[r - skip] = first + j;
        base += total;
    }
    // the old cells that stay: those with fewer than keep - nin larger old keys
    const int room = keep - nin, cpt = (keep + DP_THREADS - 1) / DP_THREADS;
    int       n_free = 0;
    uint32_t  freed = 0, evicted = 0;
#pragma unroll
    for (int q = 0; q < DP_PER_THREAD; ++q) {
        const int c = tid * cpt + q;
        if (q >= cpt || c >= keep) continue;
        const uint64_t k = L.okey[c];
        const bool     stays = k != 0 && dp_larger(L.okey, keep, k) < room;
        if (!stays) { freed |= 1u << q; ++n_free; }
        if (!stays && k != 0) evicted |= 1u << q;
    }
    int total_free;
    int rank = dp_scan(n_free, L.wsum, tid, total_free);
#pragma unroll
    for (int q = 0; q < DP_PER_THREAD; ++q) {
        if (!(freed >> q & 1u)) continue;
        const int c = tid * cpt + q;
        if (rank < nin) L.cell_of[rank] = c;
        else if (evicted >> q & 1u) key[c] = 0;          // (an evicted cell that nothing takes)
        ++rank;
    }
    __syncthreads();
    return nin;
}

// the LDS of a join's placement
struct DpJoinLds {
    uint64_t dkey[DP_MAX_KEEP], skey[DP_MAX_KEEP];
    int32_t  take[DP_MAX_KEEP];           // the i-th surviving cell of the src, ascending by key
    int32_t  cell_of[DP_MAX_KEEP];        // ... and the cell of dst it takes
    int      wsum[DP_WAVES];
};

// The placement of one src of a join, by the whole workgroup: L.dkey holds dst's keys as they are now, gkey_dst / gkey_src [keep] are
// the two slots' keys in global memory.  Returns the number of the src's survivors; L.take and L.cell_of hold them, and the evicted
// cells of dst nothing takes are emptied.  It ends on a barrier.  The caller moves the cells, sets L.dkey[cell_of[i]] = L.skey[take[i]]
// and empties the src.  The `keep` largest keys of a union are those of the union of the lists' own `keep` largest, so LDS holds the
// keys of two slots, whatever n_srcs is.
__device__ __forceinline__ int dp_place_join(DpJoinLds &L, uint64_t *gkey_dst, const uint64_t *gkey_src, int keep, int tid)
{
    const int cpt = (keep + DP_THREADS - 1) / DP_THREADS;
    __syncthreads();          // (the keys and places of the src before are read)
    for (int c = tid; c < keep; c += DP_THREADS) L.skey[c] = gkey_src[c];
    __syncthreads();
    // the src's survivors: fewer than keep larger keys in both lists
    int      n_surv = 0, larger_own[DP_PER_THREAD];
    uint32_t surv = 0;
#pragma unroll
    for (int q = 0; q < DP_PER_THREAD; ++q) {
        const int c = tid * cpt + q;
        larger_own[q] = 0;
        if (q >= cpt || c >= keep) continue;
        const uint64_t k = L.skey[c];
        if (k == 0) continue;
        larger_own[q] = dp_larger(L.skey, keep, k);
        if (larger_own[q] + dp_larger(L.dkey, keep, k) < keep) { surv |= 1u << q; ++n_surv; }
    }
    int n_in;
    dp_scan(n_surv, L.wsum, tid, n_in);
#pragma unroll
    for (int q = 0; q < DP_PER_THREAD; ++q)
        if (surv >> q & 1u) L.take[n_in - 1 - larger_own[q]] = tid * cpt + q;          // (every larger key of the src survives too)
    // the cells of dst that stay
    int      n_free = 0;
    uint32_t freed = 0, evicted = 0;
#pragma unroll
    for (int q = 0; q < DP_PER_THREAD; ++q) {
        const int c = tid * cpt + q;
        if (q >= cpt || c >= keep) continue;
        const uint64_t k = L.dkey[c];
        const bool     stays = k != 0 && dp_larger(L.dkey, keep, k) + dp_larger(L.skey, keep, k) < keep;
        if (!stays) { freed |= 1u << q; ++n_free; }
        if (!stays && k != 0) evicted |= 1u << q;
    }
    int total_free;
    int rank = dp_scan(n_free, L.wsum, tid, total_free);          // (its barriers: every count above is made before dkey changes)
#pragma unroll
    for (int q = 0; q < DP_PER_THREAD; ++q) {
        if (!(freed >> q & 1u)) continue;
        const int c = tid * cpt + q;
        if (rank < n_in) L.cell_of[rank] = c;
        else if (evicted >> q & 1u) { gkey_dst[c] = 0; L.dkey[c] = 0; }          // (an evicted cell that nothing takes)
        ++rank;
    }
    __syncthreads();
    return n_in;
}

} // namespace

} // namespace str_er
