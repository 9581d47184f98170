// er_masks.inl -- the pixel mask of a region (STR_ER_WANT_MASKS, str_er_er_masks).  Part of er_kernels.hip.
//
// The node (t, C) of SURVEY A.3 is a 4-connected component of {L <= t}; its key is a pixel of C.  A box is held as bit rows: the
// allowed row A[y] (bit x: L(x, y) <= level) and the reached row R[y], 64 pixels a word.  R starts as the key pixel and grows to a
// fixpoint: a row takes what its neighbour rows reach (R[y +- 1] & A[y]) and fills the runs of A[y] it touches with carry-chain fills.
// There is no iteration cap: every round that changes nothing ends the loop, every other round adds a pixel, so the result is exact
// for every shape.  One wave per box, three size classes:
//   k_er_masks_small   w, h <= 64: one row per lane, all in registers; neighbour rows come by lane shifts.
//   k_er_masks_big     A and R in LDS (h * ceil(w / 64) <= MASK_LDS_WORDS) or, for larger boxes, in global scratch: rows are swept
//                      top-down and bottom-up in turn until a sweep changes nothing.  A lane owns words lane, lane + 64, ... of every
//                      row -- the only lane that ever reads or writes them -- and carries cross word borders by lane shifts.

constexpr int MASK_THREADS   = 64;
constexpr int MASK_LDS_WORDS = 1024;     // 64-bit words per array (A, R): 16 KB of LDS a workgroup
constexpr int MASK_MAX_WPL   = 4;        // words per lane of a row: boxes up to 16384 pixels wide

// L(p) <= level, with L(p) = rint_half_even(float(p ^ invert) * float(1 / step)): the convertTo of src/ER.cpp:250, as the tile kernels quantise
__device__ __forceinline__ bool mask_allowed(const MaskJob &j, int x, int y, float qscale)
{
    const uint32_t v = j.pix[(size_t)(j.y + y) * (size_t)j.stride + (size_t)(j.x + x)] ^ j.invert;
    return __float2int_rn((float)v * qscale) <= (int)j.level;
}

// the runs of `a` that hold a bit of `s`, filled: towards bit 63 by the carry of a + s (it runs up through the run and stops above it),
// towards bit 0 the same on the bit-reversed words
__device__ __forceinline__ uint64_t mask_fill_up(uint64_t s, uint64_t a)
{
    s &= a;
    return (((a + s) ^ a) & a) | s;
}
__device__ __forceinline__ uint64_t mask_row_fill(uint64_t s, uint64_t a)
{
    return mask_fill_up(s, a) | __builtin_bitreverse64(mask_fill_up(__builtin_bitreverse64(s), __builtin_bitreverse64(a)));
}

__device__ __forceinline__ uint32_t mask_wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(MASK_THREADS) void k_er_masks_small(const MaskJob *__restrict__ jobs, int n, uint32_t *__restrict__ out,
                                                                 uint32_t *__restrict__ pixels, float qscale)
{
    const int lane = threadIdx.x;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const MaskJob j = jobs[i];
        const int     w = j.w, h = j.h;
        uint64_t      a = 0;
        for (int y = 0; y < h; ++y) {              // (a row of the box a ballot: the pixel of lane x, kept by lane y)
            const uint64_t row = __ballot(lane < w && mask_allowed(j, lane, y, qscale));
            if (lane == y) a = row;
        }
        const int kx = (int)(j.key % j.plane_w) - j.x, ky = (int)(j.key / j.plane_w) - j.y;
        uint64_t  r = (lane == ky && kx >= 0 && kx < w) ? (1ull << kx) & a : 0ull;      // (the host checked the key lies in the box)
        for (;;) {
            const uint64_t up = __shfl_up(r, 1), dn = __shfl_down(r, 1);
            const uint64_t v = mask_row_fill(r | (((lane > 0 ? up : 0ull) | (lane < 63 ? dn : 0ull)) & a), a);
            const bool changed = v != r;
            r = v;
            if (__ballot(changed) == 0) break;
        }
        const int pitch = (w + 31) >> 5;
        if (lane < h) {
            out[j.out_off + (size_t)lane * pitch] = (uint32_t)r;
            if (pitch == 2) out[j.out_off + (size_t)lane * pitch + 1] = (uint32_t)(r >> 32);
        }
        const uint32_t cnt = mask_wave_sum((uint32_t)__popcll(r));
        if (lane == 0) pixels[j.idx] = cnt;
    }
}

__device__ void mask_big_body(const MaskJob &j, uint64_t *A, uint64_t *R, uint32_t *__restrict__ out, uint32_t *__restrict__ pixels, float qscale)
{
    const int lane = threadIdx.x, w = j.w, h = j.h, P = (w + 63) >> 6, wpl = (P + 63) >> 6;
    for (int y = 0; y < h; ++y)
        for (int k = 0; k < P; ++k) {
            const int      x = 64 * k + lane;
            const uint64_t word = __ballot(x < w && mask_allowed(j, x, y, qscale));
            if (lane == (k & 63)) { A[(size_t)y * P + k] = word; R[(size_t)y * P + k] = 0; }
        }
    {
        const int kx = (int)(j.key % j.plane_w) - j.x, ky = (int)(j.key / j.plane_w) - j.y;
        if (kx >= 0 && kx < w && ky >= 0 && ky < h && lane == ((kx >> 6) & 63)) R[(size_t)ky * P + (kx >> 6)] = (1ull << (kx & 63)) & A[(size_t)ky * P + (kx >> 6)];
    }
    for (bool down = true;; down = !down) {
        bool     changed = false;
        uint64_t prev[MASK_MAX_WPL];        // the row the sweep did last (its words stay in the lane's registers)
#pragma unroll
        for (int m = 0; m < MASK_MAX_WPL; ++m) prev[m] = 0;
        for (int t = 0; t < h; ++t) {
            const int  y = down ? t : h - 1 - t;
            const bool has_next = t + 1 < h;
            uint64_t   a[MASK_MAX_WPL], v[MASK_MAX_WPL];
#pragma unroll
            for (int m = 0; m < MASK_MAX_WPL; ++m) {
                const int k = lane + 64 * m;
                a[m] = v[m] = 0;
                if (m < wpl && k < P) {
                    const size_t   o = (size_t)y * P + k;
                    a[m] = A[o];
                    const uint64_t nb = prev[m] | (has_next ? R[down ? o + P : o - P] : 0ull);
                    v[m] = mask_row_fill(R[o] | (nb & a[m]), a[m]);
                }
            }
            if (P > 1) {        // runs that cross a word border: bit 63 of word k seeds bit 0 of word k + 1 and bit 0 seeds bit 63 of word k - 1
                for (;;) {
                    bool more = false;
#pragma unroll
                    for (int m = 0; m < MASK_MAX_WPL; ++m) {
                        if (m >= wpl) break;
                        const uint64_t lu = __shfl_up(v[m], 1), rd = __shfl_down(v[m], 1);
                        const uint64_t l0 = m > 0 ? __shfl(v[m > 0 ? m - 1 : 0], 63) : 0ull;
                        const uint64_t r63 = m + 1 < wpl ? __shfl(v[m + 1 < MASK_MAX_WPL ? m + 1 : m], 0) : 0ull;
                        const uint64_t left = lane > 0 ? lu : l0, right = lane < 63 ? rd : r63;
                        const uint64_t s = (left >> 63) | (right << 63);
                        const uint64_t nv = mask_row_fill(v[m] | (s & a[m]), a[m]);
                        more |= nv != v[m];
                        v[m] = nv;
                    }
                    if (__ballot(more) == 0) break;
                }
            }
#pragma unroll
            for (int m = 0; m < MASK_MAX_WPL; ++m) {
                const int k = lane + 64 * m;
                if (m < wpl && k < P) {
                    const size_t o = (size_t)y * P + k;
                    changed |= v[m] != R[o];
                    R[o] = v[m];
                }
                prev[m] = v[m];
            }
        }
        if (__ballot(changed) == 0) break;
    }
    const int pitch = (w + 31) >> 5;
    uint32_t  cnt = 0;
    for (int y = 0; y < h; ++y)
        for (int k = lane; k < P; k += 64) {
            const uint64_t r = R[(size_t)y * P + k];
            const size_t   o = j.out_off + (size_t)y * pitch + 2 * (size_t)k;
            out[o] = (uint32_t)r;
            if (2 * k + 1 < pitch) out[o + 1] = (uint32_t)(r >> 32);
            cnt += (uint32_t)__popcll(r);
        }
    cnt = mask_wave_sum(cnt);
    if (lane == 0) pixels[j.idx] = cnt;
}

template <bool IN_LDS>
__global__ __launch_bounds__(MASK_THREADS) void k_er_masks_big(const MaskJob *__restrict__ jobs, int n, uint32_t *__restrict__ out,
                                                               uint32_t *__restrict__ pixels, uint64_t *scratch, float qscale)
{
    __shared__ uint64_t s_rows[IN_LDS ? 2 * MASK_LDS_WORDS : 1];
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const MaskJob j = jobs[i];
        const size_t  words = (size_t)j.h * (size_t)((j.w + 63) >> 6);
        uint64_t     *A = IN_LDS ? s_rows : scratch + j.scratch_off;
        mask_big_body(j, A, IN_LDS ? s_rows + MASK_LDS_WORDS : A + words, out, pixels, qscale);
    }
}

int mask_class(int w, int h)
{
    if (w <= 64 && h <= 64) return 0;
    return (size_t)h * (size_t)((w + 63) >> 6) <= (size_t)MASK_LDS_WORDS ? 1 : 2;
}

size_t mask_scratch_words(int w, int h)
{
    return mask_class(w, h) == 2 ? 2 * (size_t)h * (size_t)((w + 63) >> 6) : 0;
}

void launch_er_masks(hipStream_t s, const MaskJob *jobs, const int n_class[3], uint32_t *out, uint32_t *pixels, uint64_t *scratch, float qscale)
{
    const int grid_cap = 1 << 16;
    if (n_class[0] > 0)
        hipLaunchKernelGGL(k_er_masks_small, dim3(std::min(n_class[0], grid_cap)), dim3(MASK_THREADS), 0, s, jobs, n_class[0], out, pixels, qscale);
    jobs += n_class[0];
    if (n_class[1] > 0)
        hipLaunchKernelGGL(k_er_masks_big<true>, dim3(std::min(n_class[1], grid_cap)), dim3(MASK_THREADS), 0, s, jobs, n_class[1], out, pixels, scratch, qscale);
    jobs += n_class[1];
    if (n_class[2] > 0)
        hipLaunchKernelGGL(k_er_masks_big<false>, dim3(std::min(n_class[2], grid_cap)), dim3(MASK_THREADS), 0, s, jobs, n_class[2], out, pixels, scratch, qscale);
}
