// er_pyr_level.inl -- part of er_kernels.hip (included there behind er_tile_tree.inl, whose WAVE_SYNC it uses): k_pyr_level, the kernel of the one case a
// pyramid consists of -- a linear reduction with 1 < scale <= 1.5 in both directions between dword-aligned planes -- and launch_pyr_level, which sends
// every other case to k_resize.  Same arithmetic as resize_px (er_planes.inl), same bytes; about half the vector instructions of k_resize's fast form.
//
// One wave produces 256 columns x `rows` output rows and walks down them (8 rows unless the caller forces 16 or 32: taller tiles save set-up and cost more
// in the launch's last, partly filled round of waves -- profiles/pyr_level.md).  What depends on the column alone -- the four coefficient pairs, the four
// byte selectors, the lane's window column -- is made once per tile.
// The source rows come in chunks: the window of PL_CH output rows is PL_NR source rows of at most PL_WORDS - 2 dwords; a lane holds two words of each
// in registers, loaded (clamped into the plane, unconditionally) while the chunk before is computed, and writes them to LDS when that chunk is done.
//
// Horizontal pass, per source row and column: one v_perm_b32 makes (left tap | right tap << 16), one v_dot2_u32_u16 multiplies it with (a0 | a1 << 16);
// the sum is kept as h & ~15 = (h >> 4) << 4.  Vertical pass: with b << 12 in a scalar register, v_mul_hi_u32_u24 of the two is
// ((h >> 4) * b * 2^16) >> 32 = (b * (h >> 4)) >> 16, one instruction a product.  a0 + a1 = b0 + b1 = 2048 for every float32 fraction, so the result is
// at most 255 and is packed without a clamp (tests/test_pyr_level_rules.py states both).
//
// The two rows of sums live in hA / hB, which change roles from one output row to the next (the row loop is unrolled by two) -- no register moves.
// Every decision of the row loop is uniform over the wave, every loop is bounded by the tile's own constants, no lane
// leaves before the end: lanes beyond the plane's last column compute the last column's pixels and store nothing.
constexpr int PL_CH = 4;              // output rows of a chunk
constexpr int PL_NR = 7;              // source rows staged for a chunk: floor(1.5 * 3) + 1 steps from the first row's upper tap, + 1 for the last row's lower tap
constexpr int PL_WORDS = 100;         // dwords of a staged row: a window is at most PL_WORDS - 2 (a lane reads three dwords from its first tap's on)
constexpr int PL_MAX_ROWS = 32;       // a lane per row of the tile holds the row's taps and coefficients (lanes 0 .. 31)
constexpr int PL_ROWS = 8;            // the tile height launch_pyr_level takes unless one is forced: 16 and 32 lost on every level of a 1080p batch (profiles/pyr_level.md)

typedef unsigned short pl_u16x2 __attribute__((ext_vector_type(2)));

// (h * b) >> 32 of a 24-bit h in a vector register and a 24-bit b in a scalar one.  Written out: the compiler takes the 24-bit form of a 64-bit product only
// where it can see that both factors are 24-bit, and it loses sight of that for sums carried round a loop (the full v_mul_hi_u32 is a quarter-rate instruction).
__device__ __forceinline__ uint32_t pl_mulhi_u24(uint32_t h, uint32_t b)
{
    uint32_t m;
    asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(m) : "s"(b), "v"(h));
    return m;
}

template <bool FULL>
__device__ __forceinline__ void pyr_level_tile(uint32_t *s_win, const uint8_t *__restrict__ s, uint32_t sstride, uint8_t *__restrict__ d, uint32_t dstride,
                                               int tx0, int dy0, int rows, const ResizeGeom &g)
{
    const int lane = (int)threadIdx.x;
    const int dx0 = tx0 + lane * 4;
    // ---- per tile: the columns ----
    uint32_t aa[4], sel[4];
    int      sx0 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float fx = (float)((min(dx0 + k, g.dw - 1) + 0.5) * g.scale_x - 0.5);
        int   x = (int)floorf(fx);
        fx -= (float)x;
        if (x < 0) { fx = 0.f; x = 0; }
        if (x >= g.sw - 1) { fx = 0.f; x = g.sw - 1; }         // (a1 = 0: the right tap's byte is read, inside the window, and counts for nothing)
        const uint32_t a0 = (uint32_t)__float2int_rn((1.f - fx) * 2048.f), a1 = (uint32_t)__float2int_rn(fx * 2048.f);
        if (k == 0) sx0 = x;
        const uint32_t off = (uint32_t)(x - sx0);              // 0 .. 6 (launch_pyr_level checks it)
        aa[k] = a0 | a1 << 16;
        sel[k] = off | 0x0C00u | (off + 1u) << 16 | 0x0C000000u;      // v_perm_b32: byte `off`, 0, byte `off + 1`, 0
    }
    const int      base = sx0 & ~3;
    const uint32_t s0 = (uint32_t)(sx0 - base);
    const int      x_lo = __builtin_amdgcn_readfirstlane(base);        // lane 0's first tap is the tile's
    const uint32_t colb = (uint32_t)(base - x_lo);                     // byte offset of the lane's first dword in a staged row
    // ---- per tile: the rows (lane r: row dy0 + r) ----
    uint32_t row_y, row_b;
    {
        const int dy = min(dy0 + (lane & (PL_MAX_ROWS - 1)), g.dh - 1);
        float     fy = (float)((dy + 0.5) * g.scale_y - 0.5);
        const int sy = (int)floorf(fy);
        fy -= (float)sy;
        const uint32_t b0 = (uint32_t)__float2int_rn((1.f - fy) * 2048.f), b1 = (uint32_t)__float2int_rn(fy * 2048.f);
        row_y = (uint32_t)min(max(sy, 0), g.sh - 1) | (uint32_t)min(max(sy + 1, 0), g.sh - 1) << 16;
        row_b = b0 | b1 << 16;
    }
    const int n_rows = min(rows, g.dh - dy0), n_chunks = (n_rows + PL_CH - 1) / PL_CH;
    // ---- staging: words `lane` and `lane + 64` of every row of the chunk's window ----
    const uint32_t w0 = (uint32_t)lane, w1 = (uint32_t)min(lane + 64, PL_WORDS - 1);
    const uint32_t g0 = min((uint32_t)x_lo + 4u * w0, sstride - 4u), g1 = min((uint32_t)x_lo + 4u * w1, sstride - 4u);
    uint32_t v[PL_NR][2];
    auto fetch = [&](int y_first) {
        uint32_t o0 = g0, o1 = g1;
        asm volatile("" : "+v"(o0), "+v"(o1));        // (kept 32-bit up to the loads: scalar row pointer + lane offset is the load's own addressing)
#pragma unroll
        for (int j = 0; j < PL_NR; ++j) {
            const uint8_t *rp = s + (uint32_t)min(y_first + j, g.sh - 1) * sstride;        // (a plane is below 4 GB: launch_pyr_level)
            v[j][0] = *reinterpret_cast<const uint32_t *>(rp + o0);
            v[j][1] = *reinterpret_cast<const uint32_t *>(rp + o1);
        }
    };
    int win_next = (int)(__builtin_amdgcn_readlane(row_y, 0) & 0xFFFFu);
    fetch(win_next);
    uint32_t hA[4] = {0, 0, 0, 0}, hB[4] = {0, 0, 0, 0};
    int      cA = -1, cB = -1;            // source rows whose sums are in hA / hB
    auto hrow = [&](int yrel, uint32_t (&h)[4]) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(s_win) + (colb + (uint32_t)yrel * (PL_WORDS * 4)));
        const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
        const uint32_t lo = __builtin_amdgcn_alignbyte(d1, d0, s0), hi = __builtin_amdgcn_alignbyte(d2, d1, s0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t pair = __builtin_amdgcn_perm(hi, lo, sel[k]);
            h[k] = __builtin_amdgcn_udot2(__builtin_bit_cast(pl_u16x2, pair), __builtin_bit_cast(pl_u16x2, aa[k]), 0u, false) & 0xFFFFF0u;
        }
    };
#pragma unroll 1
    for (int c = 0; c < n_chunks; ++c) {
        const int win = win_next;
        WAVE_SYNC();            // (the reads of the chunk before are behind the wave: its LDS operations are carried out in the order it issues them)
#pragma unroll
        for (int j = 0; j < PL_NR; ++j) { s_win[j * PL_WORDS + w0] = v[j][0]; s_win[j * PL_WORDS + w1] = v[j][1]; }
        WAVE_SYNC();
        if (c + 1 < n_chunks) {
            win_next = (int)(__builtin_amdgcn_readlane(row_y, (c + 1) * PL_CH) & 0xFFFFu);
            fetch(win_next);
        }
        const int r_end = min((c + 1) * PL_CH, n_rows);
        // one output row: `up` / `dn` take the sums of its upper / lower source row unless they hold them already
        auto row = [&](int r, uint32_t (&up)[4], uint32_t (&dn)[4], int &c_up, int &c_dn) {
            const uint32_t ry = __builtin_amdgcn_readlane(row_y, r), rb = __builtin_amdgcn_readlane(row_b, r);
            const int      ya = (int)(ry & 0xFFFFu), yb = (int)(ry >> 16);
            const uint32_t b0s = (rb & 0xFFFu) << 12, b1s = (rb >> 16 & 0xFFFu) << 12;        // (at most 2048 << 12: 24 bits)
            if (c_up != ya) { hrow(ya - win, up); c_up = ya; }
            if (c_dn != yb) { hrow(yb - win, dn); c_dn = yb; }
            // two columns to a register: the products are below 2^11, the sums + 2 below 2^10; >> 2 leaves a column's byte in bits 0-7 / 16-23 (and two bits
            // of the upper column in bits 14-15, which the byte permute leaves behind)
            const uint32_t t01 = (pl_mulhi_u24(up[0], b0s) | pl_mulhi_u24(up[1], b0s) << 16) + (pl_mulhi_u24(dn[0], b1s) | pl_mulhi_u24(dn[1], b1s) << 16) + 0x00020002u;
            const uint32_t t23 = (pl_mulhi_u24(up[2], b0s) | pl_mulhi_u24(up[3], b0s) << 16) + (pl_mulhi_u24(dn[2], b1s) | pl_mulhi_u24(dn[3], b1s) << 16) + 0x00020002u;
            const uint32_t o = __builtin_amdgcn_perm(t23 >> 2, t01 >> 2, 0x06040200u);
            uint8_t *q = d + (uint32_t)(dy0 + r) * dstride;
            if (FULL || dx0 + 4 <= g.dw) {
                uint32_t qo = (uint32_t)dx0;
                asm volatile("" : "+v"(qo));           // (as in fetch)
                *reinterpret_cast<uint32_t *>(q + qo) = o;
            } else for (int k = 0; k < 4 && dx0 + k < g.dw; ++k) q[dx0 + k] = (uint8_t)(o >> (8 * k));
        };
        // two rows a round, hA and hB changing roles: an output row mostly starts on the source row the one before ended on (then that row's sums are where
        // this row wants them, and one source row is summed), or one further down (then both are summed anyway) -- no register moves either way
#pragma unroll 1
        for (int r = c * PL_CH; r < r_end; r += 2) {
            row(r, hA, hB, cA, cB);
            if (r + 1 < r_end) row(r + 1, hB, hA, cB, cA);
        }
    }
}

__global__ __launch_bounds__(64) void k_pyr_level(const uint8_t *__restrict__ src, int sstride, int64_t splane_pitch, int64_t sframe_pitch,
                                                  uint8_t *__restrict__ dst, int dstride, int64_t dplane_pitch, int64_t dframe_pitch,
                                                  int planes_per_frame, int rows, ResizeGeom g)
{
    __shared__ uint32_t s_win[PL_NR * PL_WORDS + 2];        // (+2: the three dwords of a lane whose first tap is in the window's last word)
    const int tx0 = blockIdx.x * 256, dy0 = blockIdx.y * rows;
    const int f = blockIdx.z / planes_per_frame, c = blockIdx.z % planes_per_frame;
    const uint8_t *s = src + (size_t)f * sframe_pitch + (size_t)c * splane_pitch;
    uint8_t       *d = dst + (size_t)f * dframe_pitch + (size_t)c * dplane_pitch;
    if (tx0 + 256 <= g.dw) pyr_level_tile<true>(s_win, s, (uint32_t)sstride, d, (uint32_t)dstride, tx0, dy0, rows, g);
    else pyr_level_tile<false>(s_win, s, (uint32_t)sstride, d, (uint32_t)dstride, tx0, dy0, rows, g);
}

// The shapes k_pyr_level takes: what the kernel relies on, checked on the geometry's own tables (the float32 taps the kernel computes) -- every quad of columns
// within 7 source bytes, every tile's window within PL_WORDS - 2 dwords, every chunk's window within PL_NR rows.
static bool pyr_level_fits(const ResizeGeom &g, int sstride, int dstride)
{
    if (g.mode != 2 || !(g.scale_x > 1.0 && g.scale_x <= 1.5 && g.scale_y > 1.0 && g.scale_y <= 1.5) || g.sh > 0xFFFF) return false;
    if ((uint64_t)g.sh * (uint64_t)sstride > 0xFFFFFFFFull || (uint64_t)g.dh * (uint64_t)dstride > 0xFFFFFFFFull) return false;
    auto sx = [&](int dx) { return std::min(std::max((int)floorf((float)((dx + 0.5) * g.scale_x - 0.5)), 0), g.sw - 1); };
    auto sy = [&](int dy) { return (int)floorf((float)((dy + 0.5) * g.scale_y - 0.5)); };
    for (int dx = 0; dx < g.dw; dx += 4)
        if (sx(std::min(dx + 3, g.dw - 1)) - sx(dx) > 6) return false;
    for (int tx0 = 0; tx0 < g.dw; tx0 += 256) {
        const int x_lo = sx(tx0) & ~3, x_hi = std::min(sx(std::min(tx0 + 255, g.dw - 1)) + 1, g.sw - 1);
        if ((x_hi - x_lo) / 4 + 1 > PL_WORDS - 2) return false;
    }
    for (int dy = 0; dy < g.dh; dy += PL_CH) {
        const int lo = std::min(std::max(sy(dy), 0), g.sh - 1), hi = std::min(std::max(sy(std::min(dy + PL_CH - 1, g.dh - 1)) + 1, 0), g.sh - 1);
        if (hi - lo + 1 > PL_NR) return false;
    }
    return true;
}

int launch_pyr_level(hipStream_t s, const uint8_t *src, int sw, int sh, int sstride, int64_t splane_pitch, int64_t sframe_pitch, uint8_t *dst, int dw, int dh,
                     int dstride, int64_t dplane_pitch, int64_t dframe_pitch, int planes_per_frame, int n_frames, int rows, bool enable)
{
    struct Seen { int sw, sh, dw, dh, sstride, dstride; bool fits; };
    thread_local Seen seen[16];                 // (a pyramid's levels: the tables are walked once per geometry and thread, not once per batch)
    thread_local int  n_seen = 0, at = 0;
    const ResizeGeom  g = host_resize_geom(sw, sh, dw, dh);
    const bool aligned = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (uintptr_t)sstride | (uintptr_t)dstride | (uintptr_t)splane_pitch |
                           (uintptr_t)sframe_pitch | (uintptr_t)dplane_pitch | (uintptr_t)dframe_pitch) & 3) == 0;
    bool fits = false;
    if (enable && aligned && sstride >= 4 && (rows == 0 || rows == 8 || rows == 16 || rows == 32)) {
        int i = 0;
        while (i < n_seen && !(seen[i].sw == sw && seen[i].sh == sh && seen[i].dw == dw && seen[i].dh == dh && seen[i].sstride == sstride && seen[i].dstride == dstride)) ++i;
        if (i == n_seen) {
            i = at; at = (at + 1) % 16; n_seen = std::min(n_seen + 1, 16);
            seen[i] = Seen{sw, sh, dw, dh, sstride, dstride, pyr_level_fits(g, sstride, dstride)};
        }
        fits = seen[i].fits;
    }
    if (!fits) {
        launch_resize(s, src, sw, sh, sstride, splane_pitch, sframe_pitch, dst, dw, dh, dstride, dplane_pitch, dframe_pitch, planes_per_frame, n_frames);
        return 0;
    }
    if (rows == 0) rows = PL_ROWS;
    dim3 grid((dw + 255) / 256, (dh + rows - 1) / rows, planes_per_frame * n_frames);
    hipLaunchKernelGGL(k_pyr_level, grid, dim3(64), 0, s, src, sstride, splane_pitch, sframe_pitch, dst, dstride, dplane_pitch, dframe_pitch, planes_per_frame,
                       rows, g);
    return rows;
}
