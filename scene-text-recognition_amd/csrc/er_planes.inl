// er_planes.inl -- part of er_kernels.hip (included there, inside namespace str_er; not a translation unit of its own): compute_channels, NV12 ingest, cv::resize (pyramid levels).
// ------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------
#define LD_AGENT(p)      __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define ST_AGENT(p, v)   __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define LD_WG(p)         __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)

__device__ __forceinline__ int find_plane_by_tile(const PlaneDesc *pl, int n, uint32_t tile)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pl[mid].tile_base <= tile) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int find_plane_by_pair(const PlaneDesc *pl, int n, uint32_t pair)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pl[mid].pair_base <= pair) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ------------------------------------------------------------------------------------
// compute_channels (src/ER.cpp:114-128): OpenCV 8-bit BGR2YCrCb, yuv_shift = 14.
// One lane converts 4 pixels: 12 bytes in (three dwords), three dwords out.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void ycrcb_px(int B, int G, int R, int &Y, int &Cr, int &Cb)
{
    Y  = (1868 * B + 9617 * G + 4899 * R + 8192) >> 14;
    Cr = ((R - Y) * 11682 + (128 << 14) + 8192) >> 14;
    Cb = ((B - Y) * 9241 + (128 << 14) + 8192) >> 14;
    Y  = min(max(Y, 0), 255);
    Cr = min(max(Cr, 0), 255);
    Cb = min(max(Cb, 0), 255);
    // Toolchain hazard (ROCm 7.2 hipcc, gfx950): when two such clamped shifts are packed into
    // bytes, LLVM fuses them into v_ashr_pk_u8_i32 and then ORs further bytes into the result
    // assuming bits 31:16 are zero -- on MI355X they keep the old register contents, which
    // corrupted byte 2 of every packed Cr/Cb dword.  The empty asm makes each value opaque so
    // the fusion cannot happen.
    asm volatile("" : "+v"(Y));
    asm volatile("" : "+v"(Cr));
    asm volatile("" : "+v"(Cb));
}

__global__ __launch_bounds__(256) void k_bgr_to_ycrcb(const uint8_t *__restrict__ bgr, int w, int h,
                                                      int64_t stride, int64_t frame_pitch,
                                                      uint8_t *__restrict__ yp, uint8_t *__restrict__ crp,
                                                      uint8_t *__restrict__ cbp, int dstride,
                                                      int64_t dst_frame_pitch, int aligned)
{
    const int quad = blockIdx.x * blockDim.x + threadIdx.x; // 4-pixel group in the row
    const int y = blockIdx.y, f = blockIdx.z;
    const int x = quad * 4;
    if (x >= w) return;
    const uint8_t *src = bgr + (size_t)f * frame_pitch + (size_t)y * stride + (size_t)x * 3;
    const size_t   dof = (size_t)f * dst_frame_pitch + (size_t)y * dstride + x;
#include "ycrcb_quad_body.inl"
}

void launch_bgr_to_ycrcb(hipStream_t s, const uint8_t *bgr, int w, int h, int64_t stride, int64_t frame_pitch,
                         int n_frames, uint8_t *y, uint8_t *cr, uint8_t *cb, int dstride, int64_t dst_frame_pitch)
{
    const int quads = (w + 3) / 4;
    const int aligned = ((reinterpret_cast<uintptr_t>(bgr) | (uintptr_t)stride | (uintptr_t)frame_pitch) % 4 == 0) &&
                        ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(cr) |
                          reinterpret_cast<uintptr_t>(cb) | (uintptr_t)dstride | (uintptr_t)dst_frame_pitch) % 4 == 0);
    dim3 grid((quads + 255) / 256, h, n_frames);
    hipLaunchKernelGGL(k_bgr_to_ycrcb, grid, dim3(256), 0, s, bgr, w, h, stride, frame_pitch, y, cr, cb, dstride,
                       dst_frame_pitch, aligned);
}

// NV12 ingest (build-defined, like the pyramid; SURVEY 8(f) row 3: "NV12 -> YCrCb directly, skipping BGR").  A decoder's frame is a
// full-resolution luma plane followed by one interleaved chroma plane at half resolution (Cb, Cr, Cb, Cr ...).  The three planes of
// the path are, by definition (oracle: ero_nv12_to_ycrcb):  Y = the luma byte;  Cr(x, y) = V(x / 2, y / 2);  Cb(x, y) = U(x / 2, y / 2)
// -- chroma replicated over its 2 x 2 block, no filter, no range conversion: the decoder's samples ARE the channel values.  Half the
// bytes of a BGR frame cross the host link.  One lane converts 4 pixels of a row: one luma dword, two chroma pairs.
__global__ __launch_bounds__(256) void k_nv12_to_ycrcb(const uint8_t *__restrict__ nv12, int w, int h, int64_t stride, int64_t frame_pitch,
                                                       uint8_t *__restrict__ yp, uint8_t *__restrict__ crp, uint8_t *__restrict__ cbp, int dstride,
                                                       int64_t dst_frame_pitch, int aligned)
{
    const int quad = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y, f = blockIdx.z;
    const int x = quad * 4;
    if (x >= w) return;
    const uint8_t *ys = nv12 + (size_t)f * frame_pitch + (size_t)y * stride + x;
    const uint8_t *uv = nv12 + (size_t)f * frame_pitch + (size_t)h * stride + (size_t)(y >> 1) * stride + x;     // (x is even: pair x / 2 starts at byte x)
    const size_t   dof = (size_t)f * dst_frame_pitch + (size_t)y * dstride + x;
#include "nv12_quad_body.inl"
}

void launch_nv12_to_ycrcb(hipStream_t s, const uint8_t *nv12, int w, int h, int64_t stride, int64_t frame_pitch, int n_frames, uint8_t *y, uint8_t *cr,
                          uint8_t *cb, int dstride, int64_t dst_frame_pitch)
{
    const int quads = (w + 3) / 4;
    const int aligned = ((reinterpret_cast<uintptr_t>(nv12) | (uintptr_t)stride | (uintptr_t)frame_pitch) % 4 == 0) &&
                        ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(cr) | reinterpret_cast<uintptr_t>(cb) | (uintptr_t)dstride |
                          (uintptr_t)dst_frame_pitch) % 4 == 0);
    dim3 grid((quads + 255) / 256, h, n_frames);
    hipLaunchKernelGGL(k_nv12_to_ycrcb, grid, dim3(256), 0, s, nv12, w, h, stride, frame_pitch, y, cr, cb, dstride, dst_frame_pitch, aligned);
}

__global__ __launch_bounds__(256) void k_invert(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += step) dst[i] = (uint8_t)(255 - src[i]);
}

void launch_invert(hipStream_t s, const uint8_t *src, uint8_t *dst, size_t n)
{
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_invert, dim3(blocks ? blocks : 1), dim3(256), 0, s, src, dst, n);
}

// ------------------------------------------------------------------------------------
// cv::resize, INTER_LINEAR, 8UC1 (OpenCV 4.x semantics; see oracle/er_oracle.c for the
// statement this follows).  `inv` is xor-ed into every tap so an inverted channel is
// resized exactly like the materialised 255-x plane would be.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ int resize_px(const ResizeGeom &g, const uint8_t *__restrict__ src, int sstride, int inv,
                                         int dx, int dy)
{
    if (g.mode == 0) return src[(size_t)dy * sstride + dx] ^ inv;
    if (g.mode == 1) {
        const uint8_t *r0 = src + (size_t)(2 * dy) * sstride + 2 * dx, *r1 = r0 + sstride;
        return ((r0[0] ^ inv) + (r0[1] ^ inv) + (r1[0] ^ inv) + (r1[1] ^ inv) + 2) >> 2;
    }
    float fx = (float)((dx + 0.5) * g.scale_x - 0.5);
    int   sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) { fx = 0.f; sx = 0; }
    if (sx >= g.sw - 1) { fx = 0.f; sx = g.sw - 1; }
    const int a0 = __float2int_rn((1.f - fx) * 2048.f), a1 = __float2int_rn(fx * 2048.f);
    float fy = (float)((dy + 0.5) * g.scale_y - 0.5);
    int   sy = (int)floorf(fy);
    fy -= (float)sy;
    const int b0 = __float2int_rn((1.f - fy) * 2048.f), b1 = __float2int_rn(fy * 2048.f);
    const int y0 = min(max(sy, 0), g.sh - 1), y1 = min(max(sy + 1, 0), g.sh - 1);
    const int sx1 = (sx + 1 < g.sw) ? sx + 1 : sx;
    const uint8_t *p0 = src + (size_t)y0 * sstride, *p1 = src + (size_t)y1 * sstride;
    const int r0 = (p0[sx] ^ inv) * a0 + (p0[sx1] ^ inv) * a1;
    const int r1 = (p1[sx] ^ inv) * a0 + (p1[sx1] ^ inv) * a1;
    const int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
    return min(max(v, 0), 255);
}

// Pyramid level: one wave per workgroup produces a 256 x 8 tile of the output.  Every lane owns 4 consecutive
// columns: their coefficients (the f64/f32 part of cv::resize's tables) are computed once and reused for the 8
// rows; one dword store per row.  The source window of the tile is first copied into LDS with coalesced dword
// loads -- byte gathers straight from global memory cost a texture-addresser pass per 4 lanes and bound the
// kernel -- and the taps are byte reads from LDS.  Windows that do not fit (large reductions, unaligned rows:
// only through str_er_resize_plane) take the taps from global memory.  The geometry is computed on the host.
constexpr int RESIZE_ROWS = 8;
constexpr int RS_WORDS = 96, RS_ROWS = 16;        // LDS window: 384 source bytes x 16 rows (a sqrt(2) step needs 364 x 14)

__device__ __forceinline__ int resize_sx(const ResizeGeom &g, int dx)
{
    const float fx = (float)((dx + 0.5) * g.scale_x - 0.5);
    return min(max((int)floorf(fx), 0), g.sw - 1);
}
__device__ __forceinline__ int resize_sy(const ResizeGeom &g, int dy)
{
    const float fy = (float)((dy + 0.5) * g.scale_y - 0.5);
    return (int)floorf(fy);
}

__global__ __launch_bounds__(64) void k_resize(const uint8_t *__restrict__ src, int sstride, int64_t splane_pitch,
                                               int64_t sframe_pitch, uint8_t *__restrict__ dst, int dstride,
                                               int64_t dplane_pitch, int64_t dframe_pitch, int planes_per_frame,
                                               ResizeGeom g)
{
    __shared__ uint32_t s_src[RS_ROWS * RS_WORDS + 2];      // (+2: a lane reads three dwords from its first tap on)
    const int tx0 = blockIdx.x * 256;
    const int dx0 = tx0 + (int)threadIdx.x * 4;
    const int dy0 = blockIdx.y * RESIZE_ROWS;
    const bool active = dx0 < g.dw;
    const int f = blockIdx.z / planes_per_frame, c = blockIdx.z % planes_per_frame;
    const uint8_t *s = src + (size_t)f * sframe_pitch + (size_t)c * splane_pitch;
    uint8_t       *d = dst + (size_t)f * dframe_pitch + (size_t)c * dplane_pitch;
#include "resize_tile_body.inl"
}

static ResizeGeom host_resize_geom(int sw, int sh, int dw, int dh)
{
    ResizeGeom g;
    g.sw = sw; g.sh = sh; g.dw = dw; g.dh = dh;
    g.scale_x = 1.0 / ((double)dw / sw);
    g.scale_y = 1.0 / ((double)dh / sh);
    if (dw == sw && dh == sh) { g.mode = 0; return g; }
    const int isx = (int)rint(g.scale_x), isy = (int)rint(g.scale_y);
    const bool fast = fabs(g.scale_x - isx) < DBL_EPSILON && fabs(g.scale_y - isy) < DBL_EPSILON;
    g.mode = (fast && isx == 2 && isy == 2) ? 1 : 2;
    return g;
}

void launch_resize(hipStream_t s, const uint8_t *src, int sw, int sh, int sstride, int64_t splane_pitch,
                   int64_t sframe_pitch, uint8_t *dst, int dw, int dh, int dstride, int64_t dplane_pitch,
                   int64_t dframe_pitch, int planes_per_frame, int n_frames)
{
    const int quads = (dw + 3) / 4;
    dim3 grid((quads + 63) / 64, (dh + RESIZE_ROWS - 1) / RESIZE_ROWS, planes_per_frame * n_frames);
    hipLaunchKernelGGL(k_resize, grid, dim3(64), 0, s, src, sstride, splane_pitch, sframe_pitch, dst, dstride,
                       dplane_pitch, dframe_pitch, planes_per_frame, host_resize_geom(sw, sh, dw, dh));
}

// ------------------------------------------------------------------------------------
// Lists of frames of different sizes (str_er_detect_bgr_list / _nv12_list): one launch converts every frame of the list, one launch per
// pyramid level resizes every frame's three planes.  The grid is the frames' workgroups back to back; a table in device memory --
// first workgroup of every job (n + 1 words), then the jobs -- tells a workgroup whose it is (a binary search over the prefix words:
// scalar loads, uniform over the workgroup).  The per-pixel work is the one of k_bgr_to_ycrcb / k_nv12_to_ycrcb / k_resize: the same text
// (*_body.inl).
// ------------------------------------------------------------------------------------
struct IngestEnt {
    const uint8_t *src;          // pixel (0, 0) of the BGR frame (NV12: of its luma plane)
    uint8_t       *y;            // pixel (0, 0) of its Y plane; Cr, Cb follow plane_pitch apart
    int64_t        stride, plane_pitch;
    int32_t        w, dstride, aligned, row_wgs;     // row_wgs: workgroups of a row (256 lanes x 4 pixels each)
    const uint8_t *uv;           // NV12: the first chroma row, h rows below src (not read by the BGR kernel)
};
struct ResizeEnt {
    const uint8_t *src;          // the job's first source / destination plane; the others follow splane_pitch / dplane_pitch apart
    uint8_t       *dst;
    int64_t        splane_pitch, dplane_pitch;
    int32_t        sstride, dstride, tiles_x, tiles;      // tiles of 256 x RESIZE_ROWS output pixels: in a row, of a plane
    ResizeGeom     g;
};

static size_t list_table_head(int n) { return ((size_t)4 * (n + 1) + 63) / 64 * 64; }

__device__ __forceinline__ int find_job(const uint32_t *first, int n, uint32_t wg)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= wg) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_bgr_to_ycrcb_list(const uint32_t *__restrict__ first, const IngestEnt *__restrict__ jobs, int n)
{
    const int f = find_job(first, n, blockIdx.x);
    const IngestEnt e = jobs[f];
    const uint32_t local = blockIdx.x - first[f];
    const int y = (int)(local / (uint32_t)e.row_wgs), xb = (int)(local - (uint32_t)y * (uint32_t)e.row_wgs);
    const int x = (xb * 256 + (int)threadIdx.x) * 4;
    const int w = e.w, aligned = e.aligned;
    if (x >= w) return;
    const uint8_t *src = e.src + (size_t)y * e.stride + (size_t)x * 3;
    uint8_t       *yp = e.y, *crp = e.y + e.plane_pitch, *cbp = e.y + 2 * e.plane_pitch;
    const size_t   dof = (size_t)y * e.dstride + x;
#include "ycrcb_quad_body.inl"
}

__global__ __launch_bounds__(256) void k_nv12_to_ycrcb_list(const uint32_t *__restrict__ first, const IngestEnt *__restrict__ jobs, int n)
{
    const int f = find_job(first, n, blockIdx.x);
    const IngestEnt e = jobs[f];
    const uint32_t local = blockIdx.x - first[f];
    const int y = (int)(local / (uint32_t)e.row_wgs), xb = (int)(local - (uint32_t)y * (uint32_t)e.row_wgs);
    const int x = (xb * 256 + (int)threadIdx.x) * 4;
    const int w = e.w, aligned = e.aligned;
    if (x >= w) return;
    const uint8_t *ys = e.src + (size_t)y * e.stride + x;
    const uint8_t *uv = e.uv + (size_t)(y >> 1) * e.stride + x;          // (x is even: pair x / 2 starts at byte x)
    uint8_t       *yp = e.y, *crp = e.y + e.plane_pitch, *cbp = e.y + 2 * e.plane_pitch;
    const size_t   dof = (size_t)y * e.dstride + x;
#include "nv12_quad_body.inl"
}

__global__ __launch_bounds__(64) void k_resize_list(const uint32_t *__restrict__ first, const ResizeEnt *__restrict__ jobs, int n)
{
    const int j = find_job(first, n, blockIdx.x);
    __shared__ uint32_t s_src[RS_ROWS * RS_WORDS + 2];      // (+2: a lane reads three dwords from its first tap on)
    const ResizeEnt &e = jobs[j];
    const ResizeGeom g = e.g;
    const uint32_t local = blockIdx.x - first[j];
    const int c = (int)(local / (uint32_t)e.tiles), t = (int)(local - (uint32_t)c * (uint32_t)e.tiles);
    const int by = t / e.tiles_x, bx = t - by * e.tiles_x;
    const int sstride = e.sstride, dstride = e.dstride;
    const int tx0 = bx * 256;
    const int dx0 = tx0 + (int)threadIdx.x * 4;
    const int dy0 = by * RESIZE_ROWS;
    const bool active = dx0 < g.dw;
    const uint8_t *s = e.src + (size_t)c * e.splane_pitch;
    uint8_t       *d = e.dst + (size_t)c * e.dplane_pitch;
#include "resize_tile_body.inl"
}

size_t ingest_table_bytes(int n) { return list_table_head(n) + sizeof(IngestEnt) * (size_t)n; }
size_t resize_table_bytes(int n) { return list_table_head(n) + sizeof(ResizeEnt) * (size_t)n; }

uint32_t build_ingest_table(const IngestJob *jobs, int n, void *out)
{
    uint32_t  *first = static_cast<uint32_t *>(out);
    IngestEnt *ent = reinterpret_cast<IngestEnt *>(static_cast<uint8_t *>(out) + list_table_head(n));
    uint32_t   at = 0;
    for (int i = 0; i < n; ++i) {
        const IngestJob &j = jobs[i];
        IngestEnt e{};
        e.src = j.src; e.y = j.dst; e.stride = j.stride; e.plane_pitch = j.plane_pitch; e.w = j.w; e.dstride = j.dstride;
        e.row_wgs = ((j.w + 3) / 4 + 255) / 256;
        e.uv = j.src + (size_t)j.h * (size_t)j.stride;
        // (per frame: a host frame staged tightly has 3 w bytes a row, a device frame the caller's pitch)
        e.aligned = ((reinterpret_cast<uintptr_t>(j.src) | (uintptr_t)j.stride) % 4 == 0) &&
                    ((reinterpret_cast<uintptr_t>(j.dst) | (uintptr_t)j.plane_pitch | (uintptr_t)j.dstride) % 4 == 0);
        first[i] = at;
        at += (uint32_t)e.row_wgs * (uint32_t)j.h;
        ent[i] = e;
    }
    first[n] = at;
    return at;
}

uint32_t build_resize_table(const ResizeJob *jobs, int n, int planes, void *out)
{
    uint32_t  *first = static_cast<uint32_t *>(out);
    ResizeEnt *ent = reinterpret_cast<ResizeEnt *>(static_cast<uint8_t *>(out) + list_table_head(n));
    uint32_t   at = 0;
    for (int i = 0; i < n; ++i) {
        const ResizeJob &j = jobs[i];
        ResizeEnt e{};
        e.src = j.src; e.dst = j.dst; e.splane_pitch = j.splane_pitch; e.dplane_pitch = j.dplane_pitch; e.sstride = j.sstride; e.dstride = j.dstride;
        e.tiles_x = ((j.dw + 3) / 4 + 63) / 64;                              // (launch_resize's grid.x ...
        e.tiles = e.tiles_x * ((j.dh + RESIZE_ROWS - 1) / RESIZE_ROWS);      //  ... times its grid.y)
        e.g = host_resize_geom(j.sw, j.sh, j.dw, j.dh);
        first[i] = at;
        at += (uint32_t)e.tiles * (uint32_t)planes;
        ent[i] = e;
    }
    first[n] = at;
    return at;
}

void launch_bgr_to_ycrcb_list(hipStream_t s, const void *d_table, int n, uint32_t n_wg)
{
    if (n_wg == 0) return;
    const uint8_t *t = static_cast<const uint8_t *>(d_table);
    hipLaunchKernelGGL(k_bgr_to_ycrcb_list, dim3(n_wg), dim3(256), 0, s, reinterpret_cast<const uint32_t *>(t),
                       reinterpret_cast<const IngestEnt *>(t + list_table_head(n)), n);
}

void launch_nv12_to_ycrcb_list(hipStream_t s, const void *d_table, int n, uint32_t n_wg)
{
    if (n_wg == 0) return;
    const uint8_t *t = static_cast<const uint8_t *>(d_table);
    hipLaunchKernelGGL(k_nv12_to_ycrcb_list, dim3(n_wg), dim3(256), 0, s, reinterpret_cast<const uint32_t *>(t),
                       reinterpret_cast<const IngestEnt *>(t + list_table_head(n)), n);
}

void launch_resize_list(hipStream_t s, const void *d_table, int n, uint32_t n_wg)
{
    if (n_wg == 0) return;
    const uint8_t *t = static_cast<const uint8_t *>(d_table);
    hipLaunchKernelGGL(k_resize_list, dim3(n_wg), dim3(64), 0, s, reinterpret_cast<const uint32_t *>(t),
                       reinterpret_cast<const ResizeEnt *>(t + list_table_head(n)), n);
}
