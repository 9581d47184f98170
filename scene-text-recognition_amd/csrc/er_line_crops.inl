// er_line_crops.inl -- the rectified image of a text line (STR_ER_WANT_LINE_CROPS / _GLYPHS, str_er_line_crops).  Part of er_kernels.hip.
//
// One workgroup per line.  The host has laid the lines out (LineCropJob: the 16.16 geometry of str_er_line_crop, the Y plane, the
// output offset); a lane makes 4 adjacent bytes of the row-major crop and writes them in one 32-bit store.  Every output byte is an
// integer bilinear sample of the plane (str_er.h); the taps come through L2: a line's source footprint is a few KB and each source
// row is read by the neighbouring rows of the crop as well.
// Glyph crops take the nearest source pixel and test it against the masks of the line's distinct members (GlyphMember, bit rows of
// the mask kernels in er_masks.inl), in member order until one holds it.

constexpr int CROP_THREADS = 256;

__device__ __forceinline__ int crop_clamp(int64_t v, int hi)
{
    return (int)(v < 0 ? 0 : (v > hi ? hi : v));
}

template <bool GLYPH>
__global__ __launch_bounds__(CROP_THREADS) void k_line_crops(const LineCropJob *__restrict__ jobs, int n, uint8_t *__restrict__ out,
                                                             uint8_t *__restrict__ glyph, const GlyphMember *__restrict__ members,
                                                             const uint32_t *__restrict__ bits)
{
    for (int li = blockIdx.x; li < n; li += gridDim.x) {
        const LineCropJob j = jobs[li];
        const int         npx = j.width * j.height, nq = (npx + 3) >> 2;
        for (int q = threadIdx.x; q < nq; q += CROP_THREADS) {
            const int e = 4 * q;
            int       row = e / j.width, col = e - row * j.width;
            uint32_t  grey4 = 0, glyph4 = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (e + b < npx) {
                    const int64_t sx = (int64_t)j.ax + (int64_t)col * j.ux + (int64_t)row * j.vx;
                    const int64_t sy = (int64_t)j.ay + (int64_t)col * j.uy + (int64_t)row * j.vy;
                    const int64_t x0 = sx >> 16, y0 = sy >> 16;
                    const int     fx = (int)((sx >> 8) & 255), fy = (int)((sy >> 8) & 255);
                    const int     xa = crop_clamp(x0, j.pw - 1), xb = crop_clamp(x0 + 1, j.pw - 1);
                    const int     ya = crop_clamp(y0, j.ph - 1), yb = crop_clamp(y0 + 1, j.ph - 1);
                    const uint8_t *ra = j.pix + (size_t)ya * (size_t)j.stride, *rb = j.pix + (size_t)yb * (size_t)j.stride;
                    const int     top = (int)ra[xa] * (256 - fx) + (int)ra[xb] * fx;
                    const int     bot = (int)rb[xa] * (256 - fx) + (int)rb[xb] * fx;
                    grey4 |= (uint32_t)((top * (256 - fy) + bot * fy + 32768) >> 16) << (8 * b);
                    if (GLYPH) {
                        const int64_t xn = (sx + 32768) >> 16, yn = (sy + 32768) >> 16;
                        bool          hit = false;
                        if (xn >= 0 && xn < j.pw && yn >= 0 && yn < j.ph)
                            for (uint32_t k = 0; k < j.m_count && !hit; ++k) {
                                const GlyphMember m = members[j.m_first + k];
                                const int         dx = (int)xn - m.x, dy = (int)yn - m.y;
                                if (dx >= 0 && dx < m.w && dy >= 0 && dy < m.h) {
                                    const uint32_t w = bits[m.word_off + (size_t)dy * ((m.w + 31u) >> 5) + (size_t)(dx >> 5)];
                                    hit = (w >> (dx & 31)) & 1u;
                                }
                            }
                        glyph4 |= (hit ? 255u : 0u) << (8 * b);
                    }
                }
                if (++col == j.width) { col = 0; ++row; }
            }
            *reinterpret_cast<uint32_t *>(out + j.out_off + (size_t)e) = grey4;
            if (GLYPH) *reinterpret_cast<uint32_t *>(glyph + j.out_off + (size_t)e) = glyph4;
        }
    }
}

void launch_line_crops(hipStream_t s, const LineCropJob *jobs, int n, uint8_t *out, uint8_t *glyph, const GlyphMember *members, const uint32_t *bits)
{
    if (n <= 0) return;
    const dim3 grid((unsigned)std::min(n, 1 << 16));
    if (glyph)
        hipLaunchKernelGGL(k_line_crops<true>, grid, dim3(CROP_THREADS), 0, s, jobs, n, out, glyph, members, bits);
    else
        hipLaunchKernelGGL(k_line_crops<false>, grid, dim3(CROP_THREADS), 0, s, jobs, n, out, glyph, members, bits);
}
