// er_text_map.inl -- the frame-resolution text map and line-id map (STR_ER_WANT_TEXT_MAP / _LINE_MAP, str_er_text_map_regions).
// Part of er_kernels.hip.
//
// A gather, one wave per tile, no atomics: a text pixel lies under dozens of nested regions of every plane and level, and a scatter
// of atomicOr per region would contend exactly there.  The host has binned the regions into tiles (TextMapTile: a run of elements of
// one frame's map, at least a row long, so the tiles a region's pre-image box reaches are exactly the ones from its first element's
// to its last's) and laid out the uint16 tables xs(x) / ys(y) of every (frame size, level size) pair of the pixel rule (str_er.h,
// str_er_frame_map), so the kernel does no division per region.  The wave walks its tile's list with scalar loads (the tile index is
// uniform), a lane holds 4 consecutive elements of each of TMAP_ROWS chunk rows of 256 elements in registers: the OR of the values
// and the min of the ids.  Every element is written once, 4 bytes / 16 bytes per lane store; tiles without regions store 0 and -1.

constexpr int TMAP_THREADS = 256;           // 4 waves, a tile each
constexpr int TMAP_ROWS    = 8;             // a chunk: 8 rows of 256 elements (TextMapTile::n_elem is walked in such chunks)
constexpr int TMAP_CHUNK   = TMAP_ROWS * 256;
static_assert(TMAP_CHUNK == (int)TMAP_CHUNK_ELEMS, "the host lays tiles out in chunks of the kernel's");

template <bool MAP, bool IDS>
__global__ __launch_bounds__(TMAP_THREADS) void k_text_map(const TextMapTile *__restrict__ tiles, int n_tiles, const uint32_t *__restrict__ list,
                                                           const TextMapCand *__restrict__ cands, const uint16_t *__restrict__ tabs,
                                                           const uint32_t *__restrict__ bits, uint8_t *__restrict__ map, int32_t *__restrict__ ids)
{
    const int lane = threadIdx.x & 63;
    for (int t0 = blockIdx.x * (TMAP_THREADS / 64); t0 < n_tiles; t0 += gridDim.x * (TMAP_THREADS / 64)) {
        const int t = __builtin_amdgcn_readfirstlane(t0 + (int)(threadIdx.x >> 6));
        if (t >= n_tiles) continue;
        const TextMapTile T = tiles[t];
        const uint32_t    W = (uint32_t)T.width, H = (uint32_t)T.height;
        for (uint32_t c0 = 0; c0 < T.n_elem; c0 += TMAP_CHUNK) {
            // (x, y) of the lane's elements: packed y << 16 | x; elements past the frame's pixels (the padding) get y = H, outside every box
            uint32_t xy[TMAP_ROWS][4];
#pragma unroll
            for (int r = 0; r < TMAP_ROWS; ++r) {
                const uint32_t e = T.e0 + c0 + (uint32_t)(256 * r + 4 * lane);
                uint32_t       y = e / W, x = e - y * W;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    xy[r][k] = y < H ? (y << 16) | x : (H << 16);
                    if (++x == W) { x = 0; ++y; }
                }
            }
            uint32_t val[TMAP_ROWS];
            int32_t  mid[TMAP_ROWS][4];
#pragma unroll
            for (int r = 0; r < TMAP_ROWS; ++r) {
                val[r] = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) mid[r][k] = INT32_MAX;
            }
            for (uint32_t i = 0; i < T.count; ++i) {
                const TextMapCand C = cands[list[T.first + i]];
#pragma unroll
                for (int r = 0; r < TMAP_ROWS; ++r)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int x = (int)(xy[r][k] & 0xFFFFu), y = (int)(xy[r][k] >> 16);
                        if (x < C.fx0 || x >= C.fx1 || y < C.fy0 || y >= C.fy1) continue;
                        const int dx = (int)tabs[C.xtab + (uint32_t)x] - C.x, dy = (int)tabs[C.ytab + (uint32_t)y] - C.y;
                        if (dx < 0 || dx >= C.w || dy < 0 || dy >= C.h) continue;        // (the pre-image is exact: never taken)
                        const uint32_t wd = bits[C.word_off + (uint64_t)dy * C.pitch + (uint32_t)(dx >> 5)];
                        if (!((wd >> (dx & 31)) & 1u)) continue;
                        if (MAP) val[r] |= C.value << (8 * k);
                        if (IDS) mid[r][k] = min(mid[r][k], C.id);
                    }
            }
#pragma unroll
            for (int r = 0; r < TMAP_ROWS; ++r) {
                const uint32_t rel = c0 + (uint32_t)(256 * r + 4 * lane);
                if (rel >= T.n_elem) continue;
                const uint64_t e = T.off + T.e0 + rel;
                if (MAP) *reinterpret_cast<uint32_t *>(map + e) = val[r];
                if (IDS) {
                    int4 v;
                    v.x = mid[r][0] == INT32_MAX ? -1 : mid[r][0];
                    v.y = mid[r][1] == INT32_MAX ? -1 : mid[r][1];
                    v.z = mid[r][2] == INT32_MAX ? -1 : mid[r][2];
                    v.w = mid[r][3] == INT32_MAX ? -1 : mid[r][3];
                    *reinterpret_cast<int4 *>(ids + e) = v;
                }
            }
        }
    }
}

void launch_text_map(hipStream_t s, const TextMapTile *tiles, int n_tiles, const uint32_t *list, const TextMapCand *cands, const uint16_t *tabs,
                     const uint32_t *bits, uint8_t *map, int32_t *ids)
{
    if (n_tiles <= 0 || (!map && !ids)) return;
    const dim3 grid((unsigned)std::min((n_tiles + TMAP_THREADS / 64 - 1) / (TMAP_THREADS / 64), 1 << 16));
    if (map && ids)
        hipLaunchKernelGGL((k_text_map<true, true>), grid, dim3(TMAP_THREADS), 0, s, tiles, n_tiles, list, cands, tabs, bits, map, ids);
    else if (map)
        hipLaunchKernelGGL((k_text_map<true, false>), grid, dim3(TMAP_THREADS), 0, s, tiles, n_tiles, list, cands, tabs, bits, map, ids);
    else
        hipLaunchKernelGGL((k_text_map<false, true>), grid, dim3(TMAP_THREADS), 0, s, tiles, n_tiles, list, cands, tabs, bits, map, ids);
}
