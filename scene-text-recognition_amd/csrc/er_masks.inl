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
// With SHAPES (STR_ER_WANT_SHAPES, str_er_er_shapes) an epilogue turns the reached rows into a ShapeRec (str_er_shape): popcounts of
// the rows and their neighbours, the row extents for the hull, a second read of the plane for the grey sums, and a second fixpoint
// flood -- the complement of the mask, 8-connected, seeded from the box border -- for the holes.  The mask-only instantiations run none of it.
// With STROKES (STR_ER_WANT_STROKES, str_er_er_strokes) another epilogue erodes the mask to nothing, 4- and 8-neighbourhoods in turn, and
// turns the depth of every pixel into a StrokeRec (str_er_stroke).  Its last step is the first whose erosion is empty (a ballot): no cap.

constexpr int MASK_THREADS   = 64;
constexpr int MASK_LDS_WORDS = 1024;     // 64-bit words per array (A, R): 16 KB of LDS a workgroup
constexpr int MASK_MAX_WPL   = 4;        // words per lane of a row: boxes up to 16384 pixels wide

// P'(x, y) of the box: the plane XOR its invert mask
__device__ __forceinline__ uint32_t mask_pixel(const MaskJob &j, int x, int y)
{
    return j.pix[(size_t)(j.y + y) * (size_t)j.stride + (size_t)(j.x + x)] ^ j.invert;
}

// L(p) <= level, with L(p) = rint_half_even(float(p ^ invert) * float(1 / step)): the convertTo of src/ER.cpp:250, as the tile kernels quantise
__device__ __forceinline__ bool mask_allowed(const MaskJob &j, int x, int y, float qscale)
{
    return __float2int_rn((float)mask_pixel(j, x, y) * qscale) <= (int)j.level;
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

template <typename T>
__device__ __forceinline__ T mask_wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the neighbour bits of word lane + 64 m of a row held as v[0 .. wpl - 1] by every lane: bit 63 of the word to the left as bit 0, bit 0
// of the word to the right as bit 63 (0 at the row's ends)
__device__ __forceinline__ uint64_t mask_word_edges(const uint64_t (&v)[MASK_MAX_WPL], int m, int wpl, int lane)
{
    const uint64_t lu = __shfl_up(v[m], 1), rd = __shfl_down(v[m], 1);
    const uint64_t l0 = m > 0 ? __shfl(v[m > 0 ? m - 1 : 0], 63) : 0ull;
    const uint64_t r63 = m + 1 < wpl ? __shfl(v[m + 1 < MASK_MAX_WPL ? m + 1 : m], 0) : 0ull;
    const uint64_t left = lane > 0 ? lu : l0, right = lane < 63 ? rd : r63;
    return (left >> 63) | (right << 63);
}

// one row a lane (boxes up to 64 x 64): r grows inside a to a fixpoint; EIGHT: through 8-neighbours (the neighbour rows dilated by one
// pixel each way before the AND with a), else 4-neighbours
template <bool EIGHT>
__device__ __forceinline__ uint64_t mask_small_flood(uint64_t r, uint64_t a, int lane)
{
    for (;;) {
        const uint64_t up = __shfl_up(r, 1), dn = __shfl_down(r, 1);
        uint64_t       nb = (lane > 0 ? up : 0ull) | (lane < 63 ? dn : 0ull);
        if constexpr (EIGHT) nb |= (nb << 1) | (nb >> 1);
        const uint64_t v = mask_row_fill(r | (nb & a), a);
        const bool changed = v != r;
        r = v;
        if (__ballot(changed) == 0) break;
    }
    return r;
}

__device__ __forceinline__ uint32_t mask_wave_min(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ uint32_t mask_wave_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o));
    return v;
}

// One side of the hull: the point (y, x) joins a monotone chain (LOWER: the lower convex hull in x, else the upper), whose entries
// y << 16 | x sit at st[0], st[2], ...; s tracks the sum over the chain's edges of (x0 + x1)(y1 - y0).  keep = false: the last point,
// accounted for but not stored.
template <bool LOWER>
__device__ __forceinline__ void shape_hull_add(uint32_t *st, int &n, int64_t &s, int64_t y, int64_t x, bool keep)
{
    while (n >= 2) {
        const uint32_t t = st[2 * (n - 1)], u = st[2 * (n - 2)];
        const int64_t  y1 = t >> 16, x1 = t & 0xFFFF, y0 = u >> 16, x0 = u & 0xFFFF;
        const int64_t  lhs = (x1 - x0) * (y - y0), rhs = (x - x0) * (y1 - y0);
        if (LOWER ? lhs < rhs : lhs > rhs) break;       // the top turns strictly: it stays
        s -= (x0 + x1) * (y1 - y0);
        --n;
    }
    if (n >= 1) {
        const uint32_t t = st[2 * (n - 1)];
        s += ((int64_t)(t & 0xFFFF) + x) * (y - (int64_t)(t >> 16));
    }
    if (keep) st[2 * n++] = (uint32_t)y << 16 | (uint32_t)x;
}

// Twice the area of the convex hull of the corners of the mask's pixel squares, by one lane, from X[y] = xl | (xr + 1) << 32, the
// extent of row y (xl = ~0u: the row is empty).  At the height y = 0 .. h the corners span [min(xl(y - 1), xl(y)), max(xr(y - 1),
// xr(y)) + 1]; the hull's left side is the lower convex hull of the left ends, its right side the upper hull of the right ends, and
// 2 * area is the right side's sum minus the left side's.  The two stacks live in X itself, as 32-bit entries (left, right) of word i:
// a chain holds at most one entry per height already read, so entry i is written after X[i] was read.
__device__ uint64_t shape_hull_area2(uint64_t *X, int h)
{
    uint32_t *st = reinterpret_cast<uint32_t *>(X);
    int       nl = 0, nr = 0;
    int64_t   sl = 0, sr = 0;
    uint32_t  pl = ~0u, pr = 0;
    for (int y = 0; y <= h; ++y) {
        const uint64_t cur = y < h ? X[y] : 0xFFFFFFFFull;
        const uint32_t cl = (uint32_t)cur, cr = (uint32_t)(cur >> 32);
        if (cl != ~0u || pl != ~0u) {
            shape_hull_add<true>(st, nl, sl, y, min(cl, pl), y < h);
            shape_hull_add<false>(st + 1, nr, sr, y, max(cr, pr), y < h);
        }
        pl = cl; pr = cr;
    }
    return (uint64_t)(sr - sl);
}

// the record of one mask from its sums (lane 0 writes it)
__device__ __forceinline__ void shape_store(ShapeRec *out, uint32_t pix, uint32_t hp, uint32_t vp, uint32_t blk, uint32_t holes,
                                            const uint32_t cr[3], uint64_t hull2, uint64_t gs, uint64_t gs2)
{
    ShapeRec s;
    s.pixels = pix;
    s.perimeter = 4 * pix - 2 * (hp + vp);
    s.euler = (int32_t)(pix - hp - vp + blk);      // vertices - edges + faces of the 4-adjacency graph (= Gray's bit-quad count)
    s.hole_pixels = holes;
    s.crossings[0] = (uint16_t)(2 * cr[0]); s.crossings[1] = (uint16_t)(2 * cr[1]); s.crossings[2] = (uint16_t)(2 * cr[2]);
    s.crossings[3] = (uint16_t)max(min(s.crossings[0], s.crossings[1]), min(max(s.crossings[0], s.crossings[1]), s.crossings[2]));
    s.hull_area2 = hull2;
    s.grey_sum = gs;
    s.grey_sum2 = gs2;
    *out = s;
}

// the record of one mask from its per-lane sums (wave sums; lane 0 writes it): k_max = K, pc = |E_{K-1}|, the ridge at depth K
__device__ __forceinline__ void stroke_store(StrokeRec *out, uint32_t k_max, uint64_t pc, uint64_t dsum, uint64_t rp, uint64_t rs, uint64_t rs2)
{
    rp += pc; rs += (uint64_t)k_max * pc; rs2 += (uint64_t)k_max * k_max * pc;
    dsum = mask_wave_sum(dsum); rp = mask_wave_sum(rp); rs = mask_wave_sum(rs); rs2 = mask_wave_sum(rs2);
    if (threadIdx.x == 0) {
        StrokeRec s;
        s.depth_max = k_max;
        s.ridge_pixels = (uint32_t)rp;
        s.depth_sum = dsum;
        s.ridge_depth_sum = rs;
        s.ridge_depth_sum2 = rs2;
        *out = s;
    }
}

// The StrokeRec of the mask r, one row a lane (boxes up to 64 x 64).  Step k + 1 holds E_{k-1} and E_k one row a lane, takes the
// neighbour rows of E_k by lane shifts, and makes E_{k+1} = E_k eroded through N_{k+1} (4-neighbours for odd k + 1: the row's
// horizontal erosion AND the rows above and below; 8-neighbours: the horizontal erosions of the three rows ANDed).  It counts |E_k| and
// the ridge at depth k, E_{k-1} & ~dilate8(E_k).  Bits outside the box are 0 in every row, so the box border erodes like any other.
__device__ __forceinline__ void stroke_small(uint64_t r, int lane, StrokeRec *__restrict__ out)
{
    uint64_t ep = 0, ec = r;                    // E_{k-1} (0 for k = 0: no pixel has depth 0), E_k
    uint64_t dsum = 0, rp = 0, rs = 0, rs2 = 0;
    for (uint32_t k = 0;; ++k) {
        const uint64_t hz = ec & (ec << 1) & (ec >> 1), hd = ec | (ec << 1) | (ec >> 1);
        const uint64_t eu = __shfl_up(ec, 1), ed = __shfl_down(ec, 1), zu = __shfl_up(hz, 1), zd = __shfl_down(hz, 1);
        const uint64_t du = __shfl_up(hd, 1), dd = __shfl_down(hd, 1);
        const bool     t = lane > 0, b = lane < 63;
        const uint64_t en = (k & 1) == 0 ? hz & (t ? eu : 0ull) & (b ? ed : 0ull) : hz & (t ? zu : 0ull) & (b ? zd : 0ull);
        const uint64_t pc = (uint64_t)__popcll(ec), pr = (uint64_t)__popcll(ep & ~(hd | (t ? du : 0ull) | (b ? dd : 0ull)));
        dsum += pc; rp += pr; rs += k * pr; rs2 += (uint64_t)k * k * pr;
        if (__ballot(en != 0) == 0) { stroke_store(out, k + 1, pc, dsum, rp, rs, rs2); return; }
        ep = ec; ec = en;
    }
}

template <bool SHAPES, bool STROKES>
__global__ __launch_bounds__(MASK_THREADS) void k_er_masks_small(const MaskJob *__restrict__ jobs, int n, uint32_t *__restrict__ out,
                                                                 uint32_t *__restrict__ pixels, ShapeRec *__restrict__ shapes, float qscale,
                                                                 StrokeRec *__restrict__ strokes)
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
        const uint64_t r = mask_small_flood<false>((lane == ky && kx >= 0 && kx < w) ? (1ull << kx) & a : 0ull, a, lane);   // (the host checked the key lies in the box)
        const int pitch = (w + 31) >> 5;
        if (lane < h) {
            out[j.out_off + (size_t)lane * pitch] = (uint32_t)r;
            if (pitch == 2) out[j.out_off + (size_t)lane * pitch + 1] = (uint32_t)(r >> 32);
        }
        const uint32_t cnt = mask_wave_sum((uint32_t)__popcll(r));
        if (lane == 0) pixels[j.idx] = cnt;
        if constexpr (SHAPES) {
            __shared__ uint64_t s_x[64];
            const uint64_t d = __shfl_down(r, 1), dn = lane < 63 ? d : 0ull, hr = r & (r >> 1);
            const uint32_t hp = mask_wave_sum((uint32_t)__popcll(hr)), vp = mask_wave_sum((uint32_t)__popcll(r & dn));
            const uint32_t blk = mask_wave_sum((uint32_t)__popcll(hr & dn & (dn >> 1)));
            const uint32_t runs = (uint32_t)__popcll(r & ~(r << 1));
            const uint32_t cr[3] = {(uint32_t)__shfl(runs, h / 6), (uint32_t)__shfl(runs, 3 * h / 6), (uint32_t)__shfl(runs, 5 * h / 6)};
            uint64_t gs = 0, gs2 = 0;
            for (int y = 0; y < h; ++y) {
                const uint64_t row = __shfl(r, y);
                if (lane < w && ((row >> lane) & 1)) { const uint64_t v = mask_pixel(j, lane, y); gs += v; gs2 += v * v; }
            }
            gs = mask_wave_sum(gs); gs2 = mask_wave_sum(gs2);
            if (lane < h) s_x[lane] = r ? (uint64_t)__builtin_ctzll(r) | (uint64_t)(64 - __builtin_clzll(r)) << 32 : 0xFFFFFFFFull;
            __syncthreads();
            const uint64_t hull2 = lane == 0 ? shape_hull_area2(s_x, h) : 0;
            // the holes: the complement inside the box, flooded through 8-neighbours from its pixels on the box border
            const uint64_t c = lane < h ? ~r & (w == 64 ? ~0ull : (1ull << w) - 1) : 0ull;
            const uint64_t seed = (lane == 0 || lane == h - 1) ? c : c & (1ull | 1ull << (w - 1));
            const uint32_t holes = mask_wave_sum((uint32_t)__popcll(c & ~mask_small_flood<true>(seed, c, lane)));
            if (lane == 0) shape_store(shapes + j.idx, cnt, hp, vp, blk, holes, cr, hull2, gs, gs2);
            __syncthreads();        // (lane 0's reads of s_x before the next box writes it)
        }
        if constexpr (STROKES) stroke_small(r, lane, strokes + j.idx);
    }
}

// A and R of a box held as rows of P words: R grows inside A to a fixpoint by sweeps, top-down and bottom-up in turn, until one changes
// nothing; EIGHT: through 8-neighbours (the neighbour rows dilated by one pixel each way before the AND with A), else 4-neighbours
template <bool EIGHT>
__device__ void mask_sweep(const uint64_t *A, uint64_t *R, int w, int h)
{
    const int lane = threadIdx.x, P = (w + 63) >> 6, wpl = (P + 63) >> 6;
    for (bool down = true;; down = !down) {
        bool     changed = false;
        uint64_t prev[MASK_MAX_WPL];        // the row the sweep did last (its words stay in the lane's registers)
#pragma unroll
        for (int m = 0; m < MASK_MAX_WPL; ++m) prev[m] = 0;
        for (int t = 0; t < h; ++t) {
            const int  y = down ? t : h - 1 - t;
            const bool has_next = t + 1 < h;
            uint64_t   a[MASK_MAX_WPL], v[MASK_MAX_WPL], nb[MASK_MAX_WPL];
#pragma unroll
            for (int m = 0; m < MASK_MAX_WPL; ++m) {
                const int k = lane + 64 * m;
                a[m] = v[m] = nb[m] = 0;
                if (m < wpl && k < P) {
                    const size_t o = (size_t)y * P + k;
                    a[m] = A[o];
                    nb[m] = prev[m] | (has_next ? R[down ? o + P : o - P] : 0ull);
                    v[m] = EIGHT ? R[o] : mask_row_fill(R[o] | (nb[m] & a[m]), a[m]);
                }
            }
            if constexpr (EIGHT) {      // (the dilation takes bits from the neighbour lanes: every lane, outside the branch above)
                uint64_t e[MASK_MAX_WPL];
#pragma unroll
                for (int m = 0; m < MASK_MAX_WPL; ++m) e[m] = m < wpl ? mask_word_edges(nb, m, wpl, lane) : 0ull;
#pragma unroll
                for (int m = 0; m < MASK_MAX_WPL; ++m) v[m] = mask_row_fill(v[m] | (((nb[m] << 1) | nb[m] | (nb[m] >> 1) | e[m]) & a[m]), a[m]);
            }
            if (P > 1) {        // runs that cross a word border: bit 63 of word k seeds bit 0 of word k + 1 and bit 0 seeds bit 63 of word k - 1
                for (;;) {
                    bool more = false;
#pragma unroll
                    for (int m = 0; m < MASK_MAX_WPL; ++m) {
                        if (m >= wpl) break;
                        const uint64_t nv = mask_row_fill(v[m] | (mask_word_edges(v, m, wpl, lane) & a[m]), a[m]);
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
}

// the ShapeRec of the mask R (pix pixels) of a box of class 1 / 2; A is free to overwrite.  Every lane reads rows of R whole here, and
// lane 0 writes the row extents into A, so the barriers order these phases against the sweeps, where a lane touches its own words only.
__device__ void shape_big(const MaskJob &j, uint64_t *A, uint64_t *R, uint32_t pix, ShapeRec *__restrict__ shapes)
{
    const int lane = threadIdx.x, w = j.w, h = j.h, P = (w + 63) >> 6, wpl = (P + 63) >> 6;
    __syncthreads();
    uint32_t  hp = 0, vp = 0, blk = 0, cr[3] = {0, 0, 0};
    const int yc[3] = {h / 6, 3 * h / 6, 5 * h / 6};
    for (int y = 0; y < h; ++y) {
        uint64_t r[MASK_MAX_WPL], d[MASK_MAX_WPL];
#pragma unroll
        for (int m = 0; m < MASK_MAX_WPL; ++m) {
            const int k = lane + 64 * m;
            r[m] = d[m] = 0;
            if (m < wpl && k < P) {
                r[m] = R[(size_t)y * P + k];
                if (y + 1 < h) d[m] = R[(size_t)(y + 1) * P + k];
            }
        }
        uint32_t runs = 0, xl = ~0u, xr = 0;
#pragma unroll
        for (int m = 0; m < MASK_MAX_WPL; ++m) {
            if (m >= wpl) break;
            const uint64_t er = mask_word_edges(r, m, wpl, lane), ed = mask_word_edges(d, m, wpl, lane);
            const uint64_t rr = (r[m] >> 1) | (er & (1ull << 63)), dr = (d[m] >> 1) | (ed & (1ull << 63)), rl = (r[m] << 1) | (er & 1ull);
            hp += (uint32_t)__popcll(r[m] & rr);
            vp += (uint32_t)__popcll(r[m] & d[m]);
            blk += (uint32_t)__popcll(r[m] & rr & d[m] & dr);
            runs += (uint32_t)__popcll(r[m] & ~rl);
            if (r[m]) {
                const uint32_t x0 = 64u * (uint32_t)(lane + 64 * m);
                xl = min(xl, x0 + (uint32_t)__builtin_ctzll(r[m]));
                xr = max(xr, x0 + 64u - (uint32_t)__builtin_clzll(r[m]));
            }
        }
        xl = mask_wave_min(xl); xr = mask_wave_max(xr);
        if (lane == 0) A[y] = (uint64_t)xl | (uint64_t)xr << 32;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (y == yc[c]) cr[c] = mask_wave_sum(runs);
    }
    hp = mask_wave_sum(hp); vp = mask_wave_sum(vp); blk = mask_wave_sum(blk);
    uint64_t gs = 0, gs2 = 0;
    for (int y = 0; y < h; ++y)
        for (int k = 0; k < P; ++k) {
            const int x = 64 * k + lane;
            if (x < w && ((R[(size_t)y * P + k] >> lane) & 1)) { const uint64_t v = mask_pixel(j, x, y); gs += v; gs2 += v * v; }
        }
    gs = mask_wave_sum(gs); gs2 = mask_wave_sum(gs2);
    __syncthreads();
    const uint64_t hull2 = lane == 0 ? shape_hull_area2(A, h) : 0;
    __syncthreads();
    // the holes: A becomes the complement inside the box, R its pixels on the box border, then R grows through 8-neighbours
    for (int y = 0; y < h; ++y)
#pragma unroll
        for (int m = 0; m < MASK_MAX_WPL; ++m) {
            const int k = lane + 64 * m;
            if (m < wpl && k < P) {
                const size_t   o = (size_t)y * P + k;
                const uint64_t c = ~R[o] & ((k < P - 1 || (w & 63) == 0) ? ~0ull : (1ull << (w & 63)) - 1);
                const uint64_t edge = (k == 0 ? 1ull : 0ull) | (k == (w - 1) >> 6 ? 1ull << ((w - 1) & 63) : 0ull);
                A[o] = c;
                R[o] = (y == 0 || y == h - 1) ? c : c & edge;
            }
        }
    mask_sweep<true>(A, R, w, h);
    uint32_t holes = 0;
    for (int y = 0; y < h; ++y)
        for (int k = lane; k < P; k += 64) holes += (uint32_t)__popcll(A[(size_t)y * P + k] & ~R[(size_t)y * P + k]);
    holes = mask_wave_sum(holes);
    if (lane == 0) shape_store(shapes + j.idx, pix, hp, vp, blk, holes, cr, hull2, gs, gs2);
}

// one row y of E_k for the stroke sweep: its words e (0 outside the sweep's rows), their horizontal erosion z and dilation d (the bits of
// the neighbour words from mask_word_edges: every lane takes part)
__device__ __forceinline__ void stroke_row(const uint64_t *Y, int y, bool in, int P, int wpl, int lane, uint64_t (&e)[MASK_MAX_WPL],
                                           uint64_t (&z)[MASK_MAX_WPL], uint64_t (&d)[MASK_MAX_WPL])
{
#pragma unroll
    for (int m = 0; m < MASK_MAX_WPL; ++m) {
        const int k = lane + 64 * m;
        e[m] = in && m < wpl && k < P ? Y[(size_t)y * P + k] : 0ull;
    }
#pragma unroll
    for (int m = 0; m < MASK_MAX_WPL; ++m) {
        const uint64_t g = m < wpl ? mask_word_edges(e, m, wpl, lane) : 0ull;
        const uint64_t l = (e[m] << 1) | (g & 1ull), r = (e[m] >> 1) | (g & (1ull << 63));
        z[m] = e[m] & l & r;
        d[m] = e[m] | l | r;
    }
}

// The StrokeRec of the mask R of a box of class 1 / 2, by one sweep a step over the two arrays: step k + 1 reads E_{k-1}[y] from X
// and E_k[y - 1 .. y + 1] from Y (three rows kept in registers as the sweep goes down), counts |E_k| and the ridge at depth k, and
// overwrites E_{k-1}[y] with E_{k+1}[y]; then X and Y trade places.  Step 1 makes E_1 in A from E_0 = M in R.  A step sweeps only the
// rows where E_{k-1} is non-empty (E_k and E_{k+1} lie inside them, and every other row of both arrays is 0): each step removes the top
// and bottom rows of the set, so the window shrinks by at least two rows a step.  A lane reads and writes only its own words, as in
// mask_sweep.  A and R are left holding two of the E_k.
__device__ void stroke_big(int w, int h, uint64_t *A, uint64_t *R, StrokeRec *__restrict__ out)
{
    const int lane = threadIdx.x, P = (w + 63) >> 6, wpl = (P + 63) >> 6;
    uint64_t *X = A, *Y = R;
    int       plo = 0, phi = h - 1, clo = 0, chi = h - 1;       // the rows of E_{k-1} (k = 0: the box) and of E_k
    uint64_t  dsum = 0, rp = 0, rs = 0, rs2 = 0;
    for (uint32_t k = 0;; ++k) {
        uint64_t e0[MASK_MAX_WPL], z0[MASK_MAX_WPL], d0[MASK_MAX_WPL], e1[MASK_MAX_WPL], z1[MASK_MAX_WPL], d1[MASK_MAX_WPL];
        uint64_t e2[MASK_MAX_WPL], z2[MASK_MAX_WPL], d2[MASK_MAX_WPL];
        stroke_row(Y, plo - 1, false, P, wpl, lane, e0, z0, d0);
        stroke_row(Y, plo, true, P, wpl, lane, e1, z1, d1);
        uint64_t pc = 0, pr = 0;
        int      nlo = h, nhi = -1;
        for (int y = plo; y <= phi; ++y) {
            stroke_row(Y, y + 1, y + 1 <= phi, P, wpl, lane, e2, z2, d2);
            bool any = false;
#pragma unroll
            for (int m = 0; m < MASK_MAX_WPL; ++m) {
                const int kk = lane + 64 * m;
                if (m < wpl && kk < P) {
                    const size_t   o = (size_t)y * P + kk;
                    const uint64_t en = (k & 1) == 0 ? z1[m] & e0[m] & e2[m] : z0[m] & z1[m] & z2[m];
                    if (k > 0) pr += (uint64_t)__popcll(X[o] & ~(d0[m] | d1[m] | d2[m]));
                    pc += (uint64_t)__popcll(e1[m]);
                    X[o] = en;
                    any |= en != 0;
                }
            }
            if (__ballot(any)) { nlo = min(nlo, y); nhi = y; }
#pragma unroll
            for (int m = 0; m < MASK_MAX_WPL; ++m) {
                e0[m] = e1[m]; z0[m] = z1[m]; d0[m] = d1[m];
                e1[m] = e2[m]; z1[m] = z2[m]; d1[m] = d2[m];
            }
        }
        dsum += pc; rp += pr; rs += k * pr; rs2 += (uint64_t)k * k * pr;
        if (nhi < 0) { stroke_store(out, k + 1, pc, dsum, rp, rs, rs2); return; }
        uint64_t *t = X; X = Y; Y = t;
        plo = clo; phi = chi; clo = nlo; chi = nhi;
    }
}

template <bool SHAPES, bool STROKES>
__device__ void mask_big_body(const MaskJob &j, uint64_t *A, uint64_t *R, uint32_t *__restrict__ out, uint32_t *__restrict__ pixels,
                              ShapeRec *__restrict__ shapes, StrokeRec *__restrict__ strokes, float qscale)
{
    const int lane = threadIdx.x, w = j.w, h = j.h, P = (w + 63) >> 6;
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
    mask_sweep<false>(A, R, w, h);
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
    if constexpr (STROKES) {
        stroke_big(w, h, A, R, strokes + j.idx);
        if constexpr (SHAPES) {
            // R = M again for the descriptors, from the words this lane wrote to `out` above (its own words: program order is enough;
            // the fence keeps the reload behind the stroke sweep's last writes to R)
            __threadfence_block();
            for (int y = 0; y < h; ++y)
                for (int k = lane; k < P; k += 64) {
                    const size_t o = j.out_off + (size_t)y * pitch + 2 * (size_t)k;
                    R[(size_t)y * P + k] = (uint64_t)out[o] | (2 * k + 1 < pitch ? (uint64_t)out[o + 1] << 32 : 0ull);
                }
        }
    }
    if constexpr (SHAPES) shape_big(j, A, R, cnt, shapes);
}

template <bool IN_LDS, bool SHAPES, bool STROKES>
__global__ __launch_bounds__(MASK_THREADS) void k_er_masks_big(const MaskJob *__restrict__ jobs, int n, uint32_t *__restrict__ out,
                                                               uint32_t *__restrict__ pixels, ShapeRec *__restrict__ shapes, uint64_t *scratch,
                                                               float qscale, StrokeRec *__restrict__ strokes)
{
    __shared__ uint64_t s_rows[IN_LDS ? 2 * MASK_LDS_WORDS : 1];
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const MaskJob j = jobs[i];
        const size_t  words = (size_t)j.h * (size_t)((j.w + 63) >> 6);
        uint64_t     *A = IN_LDS ? s_rows : scratch + j.scratch_off;
        mask_big_body<SHAPES, STROKES>(j, A, IN_LDS ? s_rows + MASK_LDS_WORDS : A + words, out, pixels, shapes, strokes, qscale);
    }
}

int mask_class(int w, int h)
{
    if (w <= 64 && h <= 64) return 0;
    return (size_t)h * (size_t)((w + 63) >> 6) <= (size_t)MASK_LDS_WORDS ? 1 : 2;
}

size_t mask_scratch_words(int w, int h)
{
    // (A and R: the stroke sweep needs no more -- it runs in them, and with SHAPES as well R is reloaded from the mask words afterwards)
    return mask_class(w, h) == 2 ? 2 * (size_t)h * (size_t)((w + 63) >> 6) : 0;
}

template <bool SHAPES, bool STROKES>
static void launch_er_masks_t(hipStream_t s, const MaskJob *jobs, const int n_class[3], uint32_t *out, uint32_t *pixels, ShapeRec *shapes,
                              StrokeRec *strokes, uint64_t *scratch, float qscale)
{
    const int grid_cap = 1 << 16;
    if (n_class[0] > 0)
        hipLaunchKernelGGL((k_er_masks_small<SHAPES, STROKES>), dim3(std::min(n_class[0], grid_cap)), dim3(MASK_THREADS), 0, s, jobs, n_class[0], out, pixels,
                           shapes, qscale, strokes);
    jobs += n_class[0];
    if (n_class[1] > 0)
        hipLaunchKernelGGL((k_er_masks_big<true, SHAPES, STROKES>), dim3(std::min(n_class[1], grid_cap)), dim3(MASK_THREADS), 0, s, jobs, n_class[1], out,
                           pixels, shapes, scratch, qscale, strokes);
    jobs += n_class[1];
    if (n_class[2] > 0)
        hipLaunchKernelGGL((k_er_masks_big<false, SHAPES, STROKES>), dim3(std::min(n_class[2], grid_cap)), dim3(MASK_THREADS), 0, s, jobs, n_class[2], out,
                           pixels, shapes, scratch, qscale, strokes);
}

void launch_er_masks(hipStream_t s, const MaskJob *jobs, const int n_class[3], uint32_t *out, uint32_t *pixels, ShapeRec *shapes, StrokeRec *strokes,
                     uint64_t *scratch, float qscale)
{
    if (shapes && strokes) launch_er_masks_t<true, true>(s, jobs, n_class, out, pixels, shapes, strokes, scratch, qscale);
    else if (shapes)       launch_er_masks_t<true, false>(s, jobs, n_class, out, pixels, shapes, strokes, scratch, qscale);
    else if (strokes)      launch_er_masks_t<false, true>(s, jobs, n_class, out, pixels, shapes, strokes, scratch, qscale);
    else                   launch_er_masks_t<false, false>(s, jobs, n_class, out, pixels, shapes, strokes, scratch, qscale);
}
