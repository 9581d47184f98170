// er_frame_lines.inl -- the footprints of the text lines in frame pixels and their pairwise overlaps (STR_ER_WANT_FRAME_LINES,
// str_er_line_feet_regions).  Part of er_kernels.hip.
//
// k_line_foot: the footprint of every line (str_er.h, str_er_line_foot) as bit rows over the union of its members' pre-image boxes.
// A gather without atomics on pixels, for the reason er_text_map.inl gives: the members of a line come from every channel of its
// level and nest, so they cover the same pixels many times.  The host has cut every footprint into jobs of whole rows (FootJob); a
// wave takes a job, a lane the 64-bit words lane, lane + 64, ... of the job's rows.  Per member (a scalar walk: the line is uniform
// in the wave) the lane clips its word against the member's pre-image box, looks xs / ys up in the uint16 tables of the text-map
// stage (no division per pixel), reads the mask bit and ORs it in.  Every word is written once.  The wave adds up the popcounts and
// the extent of its set bits and leaves them in the line's FootStat: five atomics per job, none per pixel.
//
// k_foot_pairs: a wave takes a line a and walks the later lines b of a's frame (FootLine::next .. end, scalar); where the two
// boxes intersect it ANDs the two footprints over the intersection -- their x origins differ, so each lane funnels two words of a
// row into the 64 bits that start at the intersection's column -- popcounts and reduces.  Pairs without a common pixel are dropped
// here; lane 0 appends the others to the output (an atomic per surviving pair).  The order of the output is the order of arrival:
// the host sorts it.
//
// k_foot_links (STR_ER_WANT_LINE_LINKS, str_er_link_feet): the same walk across frames.  A wave takes a line a and walks the lines b of
// the next adjacent frame -- range[a] = (first, end) into the same list, empty where the next frame has another size or there is
// none -- with the box test fused in; a and b are in the same pixel coordinates, so the AND over the intersection is that of
// k_foot_pairs (foot_overlap).  One wave per line was kept over one wave per candidate pair: see DESIGN.md 3.15.
//
// k_foot_geom (STR_ER_WANT_LINE_GEOM, str_er_feet_geom; the contract is at str_er_line_geom): the moments and the convex hull of every
// footprint, read once.  A wave (a workgroup of its own) takes a line; a lane the rows lane, lane + 64, ... of its bit rows (a lane
// walks a whole row: the loads of neighbouring lanes lie 8 * pitch bytes apart, contiguous only where pitch is 1).  Per row
// the lane finds the extent with ctz / clz over the row's words, and per word the popcount and the sums of x and x^2 under its bits
// as bit-sliced sums (foot_word_sums: 27 popcounts, no loop over pixels); rows without a bit add nothing and leave the "empty" extent.
// The six moments are wave-reduced.  Lane 0 then runs the two monotone chains of shape_hull_area2 (er_masks.inl, shape_hull_add) over
// the row extents -- in LDS for a line of up to GEOM_LDS_ROWS - 1 rows, else in scratch words the host reserved -- keeping the last
// point as well, and the wave writes the vertices out: left[0], the right chain downwards, the left chain upwards.  The chains were
// kept sequential on one lane over a divide-and-merge of lane-local chains: see DESIGN.md 3.16.
//
// k_foot_words (STR_ER_WANT_LINE_WORDS, str_er_feet_words; the contract is at str_er_line_run): the glyph runs of every footprint.  A wave
// (a workgroup of its own) takes a line; a lane the word columns lane, lane + 64, ... of its bit rows, so the loads of neighbouring
// lanes are neighbouring words of a row.  Pass 1: the lane walks down the rows of its word column, ORs them into the column's
// occupancy word and adds every row word to 64 column counts kept bit-sliced in 15 planes (a ripple of AND / XOR that stops when the
// carry is 0); the largest of the 64 counts falls out of one descent from the top plane, colmax is a wave max.  The occupancy row
// (at most 256 words) lies in LDS: run starts are m & ~(m << 1 | carry in), run ends the mirror image, both numbered by popcounts and
// a wave prefix sum, so that the k-th start and the k-th end fill slot k whatever number of words the run or the gap before it spans.
// Pass 2: the lane walks its word column once per interval of its occupancy word -- the popcount under the interval's bits and the
// rows that have one -- and adds the result to the run's slot: in LDS (ds_add / ds_min / ds_max) for a line of up to WORDS_LDS_RUNS
// runs, else with atomics on the run's output slot.  See DESIGN.md 3.17.
//
// k_run_tiles (STR_ER_WANT_RUN_READ, str_er_feet_read; the contract is at str_er_run_read): the glyph runs as byte tiles for the OCR scorer.
// A wave takes a run; a lane four pixels of a tile row, lane after lane along the row and then down the rows, so that the stores of a
// wave are consecutive dwords of the tile's rows.  The four bits come out of the footprint row with one shift, merged with the next
// word once where they straddle it, and are spread into four bytes by shifts and one multiply.  See DESIGN.md 3.18.

constexpr int FOOT_THREADS = 256;           // 4 waves, a job / a line each

template <typename T>
__device__ __forceinline__ T foot_wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ uint32_t foot_wave_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

// the 64 bits of a footprint row (pitch words) from bit `off` on; what lies past the row is 0
__device__ __forceinline__ uint64_t foot_window(const uint64_t *__restrict__ row, uint32_t pitch, uint32_t off)
{
    const uint32_t q = off >> 6, s = off & 63u;
    uint64_t       v = q < pitch ? row[q] >> s : 0ull;
    if (s && q + 1 < pitch) v |= row[q + 1] << (64u - s);
    return v;
}

__global__ __launch_bounds__(FOOT_THREADS) void k_line_foot(const FootJob *__restrict__ jobs, int n_jobs, const FootLine *__restrict__ lines,
                                                            const TextMapCand *__restrict__ members, const uint16_t *__restrict__ tabs,
                                                            const uint32_t *__restrict__ bits, uint64_t *__restrict__ feet, FootStat *__restrict__ stat)
{
    const int lane = threadIdx.x & 63;
    const int j = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (FOOT_THREADS / 64) + (threadIdx.x >> 6)));
    if (j >= n_jobs) return;
    const FootJob  J = jobs[j];
    const FootLine L = lines[J.line];
    const uint32_t items = J.n_rows * L.pitch;
    uint32_t px = 0, nx0 = 0, ny0 = 0, x1 = 0, y1 = 0;
    for (uint32_t it = (uint32_t)lane; it < items; it += 64) {
        const uint32_t r = it / L.pitch, k = it - r * L.pitch;
        const int      y = L.y + (int)(J.row0 + r), xb = L.x + (int)(64u * k), xe = min(xb + 64, L.x + L.w);
        uint64_t       word = 0;
        for (uint32_t m = 0; m < L.count; ++m) {
            const TextMapCand C = members[L.first + m];
            if (y < C.fy0 || y >= C.fy1) continue;
            const int a = max(xb, C.fx0), e = min(xe, C.fx1);
            if (a >= e) continue;
            const int dy = (int)tabs[C.ytab + (uint32_t)y] - C.y;
            if (dy < 0 || dy >= C.h) continue;                                  // (the pre-image is exact: never taken)
            const uint32_t *row = bits + C.word_off + (uint64_t)dy * C.pitch;
            for (int x = a; x < e; ++x) {
                const int dx = (int)tabs[C.xtab + (uint32_t)x] - C.x;
                if (dx < 0 || dx >= C.w) continue;                              // (likewise)
                word |= (uint64_t)((row[dx >> 5] >> (dx & 31)) & 1u) << (x - xb);
            }
        }
        feet[L.word_off + (uint64_t)(J.row0 + r) * L.pitch + k] = word;
        if (word) {
            px += (uint32_t)__popcll(word);
            nx0 = max(nx0, 65536u - (uint32_t)(xb + (int)__builtin_ctzll(word)));
            x1 = max(x1, (uint32_t)(xb + 64 - (int)__builtin_clzll(word)));
            ny0 = max(ny0, 65536u - (uint32_t)y);
            y1 = max(y1, (uint32_t)y + 1u);
        }
    }
    px = foot_wave_sum(px);
    nx0 = foot_wave_max(nx0); ny0 = foot_wave_max(ny0); x1 = foot_wave_max(x1); y1 = foot_wave_max(y1);
    if (lane == 0 && px) {
        FootStat *S = stat + J.line;
        atomicAdd(&S->pixels, px);
        atomicMax(&S->nx0, nx0); atomicMax(&S->ny0, ny0); atomicMax(&S->x1, x1); atomicMax(&S->y1, y1);
    }
}

__global__ __launch_bounds__(FOOT_THREADS) void k_foot_pairs(const FootLine *__restrict__ lines, int n_lines, const uint32_t *__restrict__ list,
                                                             const uint64_t *__restrict__ feet, FootHead *__restrict__ head, FootPair *__restrict__ out,
                                                             uint32_t cap)
{
    const int lane = threadIdx.x & 63;
    for (int a0 = blockIdx.x * (FOOT_THREADS / 64); a0 < n_lines; a0 += gridDim.x * (FOOT_THREADS / 64)) {
        const int a = __builtin_amdgcn_readfirstlane(a0 + (int)(threadIdx.x >> 6));
        if (a >= n_lines) continue;
        const FootLine A = lines[a];
        if (A.w <= 0) continue;
        uint32_t n_cand = 0;
        for (uint32_t i = A.next; i < A.end; ++i) {
            const int      b = (int)list[i];
            const FootLine B = lines[b];
            const int ix0 = max(A.x, B.x), ix1 = min(A.x + A.w, B.x + B.w), iy0 = max(A.y, B.y), iy1 = min(A.y + A.h, B.y + B.h);
            if (ix0 >= ix1 || iy0 >= iy1) continue;
            ++n_cand;
            const uint32_t nw = (uint32_t)(ix1 - ix0 + 63) >> 6, items = (uint32_t)(iy1 - iy0) * nw;
            uint32_t inter = 0;
            for (uint32_t it = (uint32_t)lane; it < items; it += 64) {
                const uint32_t r = it / nw, k = it - r * nw;
                const int      y = iy0 + (int)r;
                const uint64_t wa = foot_window(feet + A.word_off + (uint64_t)(y - A.y) * A.pitch, A.pitch, (uint32_t)(ix0 - A.x) + 64u * k);
                const uint64_t wb = foot_window(feet + B.word_off + (uint64_t)(y - B.y) * B.pitch, B.pitch, (uint32_t)(ix0 - B.x) + 64u * k);
                inter += (uint32_t)__popcll(wa & wb);         // (past ix1 one of the two rows has ended: its bits are 0)
            }
            inter = foot_wave_sum(inter);
            if (lane == 0 && inter) {
                const uint32_t at = atomicAdd(&head->n_pairs, 1u);
                if (at < cap) { FootPair P; P.a = a; P.b = b; P.inter = inter; P.dup = 0; out[at] = P; }
            }
        }
        if (lane == 0 && n_cand) atomicAdd(&head->n_candidates, n_cand);
    }
}

// |F(a) & F(b)| over the intersection (ix0 .. ix1) x (iy0 .. iy1) of the two boxes, summed over the wave
__device__ __forceinline__ uint32_t foot_overlap(const uint64_t *__restrict__ feet, const FootLine &A, const FootLine &B, int ix0, int ix1, int iy0, int iy1,
                                                 int lane)
{
    const uint32_t nw = (uint32_t)(ix1 - ix0 + 63) >> 6, items = (uint32_t)(iy1 - iy0) * nw;
    uint32_t inter = 0;
    for (uint32_t it = (uint32_t)lane; it < items; it += 64) {
        const uint32_t r = it / nw, k = it - r * nw;
        const int      y = iy0 + (int)r;
        const uint64_t wa = foot_window(feet + A.word_off + (uint64_t)(y - A.y) * A.pitch, A.pitch, (uint32_t)(ix0 - A.x) + 64u * k);
        const uint64_t wb = foot_window(feet + B.word_off + (uint64_t)(y - B.y) * B.pitch, B.pitch, (uint32_t)(ix0 - B.x) + 64u * k);
        inter += (uint32_t)__popcll(wa & wb);         // (past ix1 one of the two rows has ended: its bits are 0)
    }
    return foot_wave_sum(inter);
}

__global__ __launch_bounds__(FOOT_THREADS) void k_foot_links(const FootLine *__restrict__ lines, int n_lines, const FootRange *__restrict__ range,
                                                             const uint32_t *__restrict__ list, const uint64_t *__restrict__ feet,
                                                             FootHead *__restrict__ head, FootPair *__restrict__ out, uint32_t cap)
{
    const int lane = threadIdx.x & 63;
    for (int a0 = blockIdx.x * (FOOT_THREADS / 64); a0 < n_lines; a0 += gridDim.x * (FOOT_THREADS / 64)) {
        const int a = __builtin_amdgcn_readfirstlane(a0 + (int)(threadIdx.x >> 6));
        if (a >= n_lines) continue;
        const FootLine A = lines[a];
        const FootRange R = range[a];
        if (A.w <= 0) continue;
        uint32_t n_cand = 0;
        for (uint32_t i = R.first; i < R.end; ++i) {
            const int      b = (int)list[i];
            const FootLine B = lines[b];
            const int ix0 = max(A.x, B.x), ix1 = min(A.x + A.w, B.x + B.w), iy0 = max(A.y, B.y), iy1 = min(A.y + A.h, B.y + B.h);
            if (ix0 >= ix1 || iy0 >= iy1) continue;
            ++n_cand;
            const uint32_t inter = foot_overlap(feet, A, B, ix0, ix1, iy0, iy1, lane);
            if (lane == 0 && inter) {
                const uint32_t at = atomicAdd(&head->n_pairs, 1u);
                if (at < cap) { FootPair P; P.a = a; P.b = b; P.inter = inter; P.dup = 0; out[at] = P; }
            }
        }
        if (lane == 0 && n_cand) atomicAdd(&head->n_candidates, n_cand);
    }
}

constexpr int GEOM_THREADS = 64;            // one wave a workgroup: the barrier between the lanes' rows and lane 0's chains is the wave's own

// of the set bits b of w: their number, the sum of b and the sum of b^2, from popcounts under the six masks "bit k of b is set"
__device__ __forceinline__ void foot_word_sums(uint64_t w, uint32_t &n, uint32_t &s1, uint32_t &s2)
{
    constexpr uint64_t M[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull, 0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull,
                               0xFFFFFFFF00000000ull};
    n = (uint32_t)__popcll(w);
    s1 = 0; s2 = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint64_t wk = w & M[k];
        const uint32_t pk = (uint32_t)__popcll(wk);
        s1 += pk << k;
        s2 += pk << (2 * k);
#pragma unroll
        for (int j = k + 1; j < 6; ++j) s2 += (uint32_t)__popcll(wk & M[j]) << (k + j + 1);
    }
}

__global__ __launch_bounds__(GEOM_THREADS) void k_foot_geom(const FootLine *__restrict__ lines, int n_lines, const GeomSlot *__restrict__ slots,
                                                            const uint64_t *__restrict__ feet, uint64_t *__restrict__ scratch, GeomRec *__restrict__ recs,
                                                            int32_t *__restrict__ xy)
{
    __shared__ uint64_t s_x[GEOM_LDS_ROWS];
    const int lane = threadIdx.x;
    for (int a = blockIdx.x; a < n_lines; a += gridDim.x) {
        const FootLine L = lines[a];
        const GeomSlot S = slots[a];
        if (L.w <= 0 || L.h <= 0) {
            if (lane == 0) recs[a] = GeomRec{0, 0, 0, 0, 0, 0, 0};
            continue;
        }
        const int h = L.h;
        // X[y] = xl | (xr + 1) << 32 relative to the box, 0xFFFFFFFF for a row without a bit; word h is the chains' last entry
        uint64_t *X = h + 1 <= GEOM_LDS_ROWS ? s_x : scratch + S.x_first;
        uint64_t n = 0, sx = 0, sy = 0, sxx = 0, sxy = 0, syy = 0;
        for (int r = lane; r < h; r += 64) {
            const uint64_t *row = feet + L.word_off + (uint64_t)r * L.pitch;
            uint32_t xl = ~0u, xr = 0;
            uint64_t cnt = 0, s1 = 0, s2 = 0;
            for (uint32_t k = 0; k < L.pitch; ++k) {
                const uint64_t w = row[k];
                if (!w) continue;
                if (xl == ~0u) xl = 64u * k + (uint32_t)__builtin_ctzll(w);
                xr = 64u * k + 64u - (uint32_t)__builtin_clzll(w);
                uint32_t p, b1, b2;
                foot_word_sums(w, p, b1, b2);
                const uint64_t xb = (uint64_t)L.x + 64u * k;
                cnt += p; s1 += p * xb + b1; s2 += p * xb * xb + 2u * xb * b1 + b2;
            }
            X[r] = (uint64_t)xl | (uint64_t)xr << 32;
            const uint64_t y = (uint64_t)L.y + (uint64_t)r;
            n += cnt; sx += s1; sxx += s2; sy += cnt * y; sxy += s1 * y; syy += cnt * y * y;
        }
        n = foot_wave_sum(n); sx = foot_wave_sum(sx); sy = foot_wave_sum(sy); sxx = foot_wave_sum(sxx); sxy = foot_wave_sum(sxy); syy = foot_wave_sum(syy);
        __syncthreads();
        int nl = 0, nr = 0;
        if (lane == 0) {
            uint32_t *st = reinterpret_cast<uint32_t *>(X);
            int64_t   sl = 0, sr = 0;
            uint32_t  pl = ~0u, pr = 0;
            for (int y = 0; y <= h; ++y) {
                const uint64_t cur = y < h ? X[y] : 0xFFFFFFFFull;
                const uint32_t cl = (uint32_t)cur, cr = (uint32_t)(cur >> 32);
                if (cl != ~0u || pl != ~0u) {
                    shape_hull_add<true>(st, nl, sl, y, min(cl, pl), true);
                    shape_hull_add<false>(st + 1, nr, sr, y, max(cr, pr), true);
                }
                pl = cl; pr = cr;
            }
            recs[a] = GeomRec{(uint32_t)(nl + nr), (uint32_t)n, sx, sy, sxx, sxy, syy};
        }
        nl = __shfl(nl, 0); nr = __shfl(nr, 0);
        __syncthreads();
        // clockwise on screen from the smallest (y, x): the top of the left chain, the right chain downwards, the left chain upwards
        const uint32_t *st = reinterpret_cast<const uint32_t *>(X);
        for (int i = lane; i < nl + nr; i += 64) {
            const uint32_t e = i == 0 ? st[0] : i <= nr ? st[2 * (i - 1) + 1] : st[2 * (nl + nr - i)];
            int32_t *o = xy + 2 * ((size_t)S.pt_first + (size_t)i);
            o[0] = L.x + (int32_t)(e & 0xFFFFu); o[1] = L.y + (int32_t)(e >> 16);
        }
        __syncthreads();        // (the wave's reads of X before the next line writes it)
    }
}

constexpr int WORDS_THREADS = 64;           // one wave a workgroup, as k_foot_geom
constexpr int WORDS_PLANES = 15;            // column counts up to WORDS_MAX_BOX = 2^14
constexpr int WORDS_MAX_PITCH = WORDS_MAX_BOX / 64;

// the inclusive prefix sum of v over the lanes of the wave
__device__ __forceinline__ uint32_t foot_wave_scan(uint32_t v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// planes K0 .. K1 - 1 of a bit-sliced add: carry is added at plane K0, what is left of it comes back
template <int K0, int K1>
__device__ __forceinline__ void foot_ripple(uint64_t (&p)[WORDS_PLANES], uint64_t &carry)
{
#pragma unroll
    for (int k = K0; k < K1; ++k) {
        const uint64_t t = p[k] & carry;
        p[k] ^= carry;
        carry = t;
    }
}

__global__ __launch_bounds__(WORDS_THREADS) void k_foot_words(const FootLine *__restrict__ lines, int n_lines, const WordsSlot *__restrict__ slots,
                                                              const uint64_t *__restrict__ feet, WordsRec *__restrict__ recs, WordsRun *__restrict__ runs)
{
    __shared__ uint64_t s_occ[WORDS_MAX_PITCH];          // the occupancy row: bit i of word j: column 64 j + i has a pixel
    __shared__ uint32_t s_base[WORDS_MAX_PITCH];         // the run of the first interval of word j
    __shared__ uint32_t s_px[WORDS_LDS_RUNS];
    __shared__ int32_t  s_y0[WORDS_LDS_RUNS], s_y1[WORDS_LDS_RUNS];
    const int lane = threadIdx.x;
    for (int a = blockIdx.x; a < n_lines; a += gridDim.x) {
        const FootLine  L = lines[a];
        const WordsSlot S = slots[a];
        if (L.w <= 0 || L.h <= 0 || L.w > WORDS_MAX_BOX || L.h > WORDS_MAX_BOX || L.pitch > (uint32_t)WORDS_MAX_PITCH) {
            if (lane == 0) recs[a] = WordsRec{0, 0};
            continue;
        }
        const uint32_t  P = L.pitch;
        const uint64_t *box = feet + L.word_off;
        // pass 1: the occupancy word and the largest column count of every word column
        uint32_t cmax = 0;
        for (uint32_t j = (uint32_t)lane; j < P; j += 64) {
            uint64_t p[WORDS_PLANES];
#pragma unroll
            for (int k = 0; k < WORDS_PLANES; ++k) p[k] = 0;
            uint64_t occ = 0;
            for (int r = 0; r < L.h; ++r) {
                uint64_t carry = box[(uint64_t)r * P + j];
                occ |= carry;
                // (planes 0 .. 1 always, the others only while a carry is left: two steps on average; every index is a constant)
                foot_ripple<0, 2>(p, carry);
                if (carry) {
                    foot_ripple<2, 4>(p, carry);
                    if (carry) {
                        foot_ripple<4, 8>(p, carry);
                        if (carry) foot_ripple<8, WORDS_PLANES>(p, carry);
                    }
                }
            }
            s_occ[j] = occ;
            uint64_t cand = occ;
            uint32_t v = 0;
#pragma unroll
            for (int k = WORDS_PLANES - 1; k >= 0; --k) {
                const uint64_t t = cand & p[k];
                if (t) { cand = t; v |= 1u << k; }
            }
            cmax = max(cmax, v);
        }
        cmax = foot_wave_max(cmax);
        __syncthreads();
        // the starts and the ends of the runs, numbered along the row: the k-th start and the k-th end are run k
        uint32_t n_st = 0, n_en = 0;
        for (uint32_t j0 = 0; j0 < P; j0 += 64) {
            const uint32_t j = j0 + (uint32_t)lane;
            uint64_t st = 0, en = 0;
            uint32_t cont = 0;          // the word's first interval goes on from the word before
            if (j < P) {
                const uint64_t m = s_occ[j];
                const uint64_t prev = j > 0 ? s_occ[j - 1] >> 63 : 0ull, next = j + 1 < P ? s_occ[j + 1] & 1ull : 0ull;
                st = m & ~(m << 1 | prev);
                en = m & ~(m >> 1 | next << 63);
                cont = (uint32_t)(prev & m);
            }
            const uint32_t ns = (uint32_t)__popcll(st), ne = (uint32_t)__popcll(en);
            const uint32_t is = foot_wave_scan(ns, lane), ie = foot_wave_scan(ne, lane);
            uint32_t ks = n_st + is - ns, ke = n_en + ie - ne;
            if (j < P) s_base[j] = ks - cont;
            for (; st; st &= st - 1, ++ks)
                if (ks < S.cap) runs[S.first + ks].x0 = L.x + (int32_t)(64u * j) + (int32_t)__builtin_ctzll(st);
            for (; en; en &= en - 1, ++ke)
                if (ke < S.cap) runs[S.first + ke].x1 = L.x + (int32_t)(64u * j) + (int32_t)__builtin_ctzll(en) + 1;
            n_st += (uint32_t)__shfl((int)is, 63); n_en += (uint32_t)__shfl((int)ie, 63);
        }
        const uint32_t n_runs = min(n_st, S.cap);         // (n_st <= (w + 1) / 2 = cap: the bits past w are 0)
        const bool     in_lds = n_runs <= (uint32_t)WORDS_LDS_RUNS;
        for (uint32_t k = (uint32_t)lane; k < n_runs; k += 64) {
            if (in_lds) { s_px[k] = 0; s_y0[k] = 0x7FFFFFFF; s_y1[k] = 0; }
            else { WordsRun *R = runs + S.first + k; R->y0 = 0x7FFFFFFF; R->y1 = 0; R->pixels = 0; R->word = -1; }
        }
        if (!in_lds) __threadfence();          // (the slots' first values ahead of the atomics on them)
        __syncthreads();
        // pass 2: per interval of the lane's occupancy word, the pixels under it and the rows that have one
        for (uint32_t j = (uint32_t)lane; j < P; j += 64) {
            uint64_t m = s_occ[j];
            uint32_t idx = s_base[j];
            for (; m; ++idx) {
                const int      b = __builtin_ctzll(m);
                const uint64_t z = ~(m >> b);
                const int      len = z ? __builtin_ctzll(z) : 64;
                const uint64_t mask = (len == 64 ? ~0ull : (1ull << len) - 1ull) << b;
                uint32_t px = 0;
                int      y0 = L.h, y1 = 0;
                for (int r = 0; r < L.h; ++r) {
                    const uint64_t w = box[(uint64_t)r * P + j] & mask;
                    if (w) { px += (uint32_t)__popcll(w); y0 = min(y0, r); y1 = r + 1; }
                }
                m &= ~mask;
                if (idx >= n_runs) continue;
                if (in_lds) {
                    atomicAdd(&s_px[idx], px); atomicMin(&s_y0[idx], L.y + y0); atomicMax(&s_y1[idx], L.y + y1);
                } else {
                    WordsRun *R = runs + S.first + idx;
                    atomicAdd(&R->pixels, px); atomicMin(&R->y0, L.y + y0); atomicMax(&R->y1, L.y + y1);
                }
            }
        }
        __syncthreads();
        if (in_lds)
            for (uint32_t k = (uint32_t)lane; k < n_runs; k += 64) {
                WordsRun *R = runs + S.first + k;
                R->y0 = s_y0[k]; R->y1 = s_y1[k]; R->pixels = s_px[k]; R->word = -1;
            }
        if (lane == 0) recs[a] = WordsRec{n_runs, cmax};
        __syncthreads();        // (the wave's reads of the LDS rows before the next line writes them)
    }
}

constexpr int TILES_THREADS = 256;          // 4 waves, a run each

__global__ __launch_bounds__(TILES_THREADS) void k_run_tiles(const RunTile *__restrict__ tiles, int n_tiles, const uint64_t *__restrict__ feet,
                                                             uint8_t *__restrict__ atlas, uint32_t stride)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int a = blockIdx.x * (TILES_THREADS / 64) + wave; a < n_tiles; a += gridDim.x * (TILES_THREADS / 64)) {
        const RunTile   T = tiles[a];
        const uint32_t  wd = (T.w + 3u) / 4u, total = wd * T.h;         // dwords of a tile row, of the tile (at most 2^12 x 2^14)
        const uint64_t *box = feet + T.bit_off;
        uint8_t        *out = atlas + (size_t)T.ay * stride + T.ax;
        for (uint32_t i = (uint32_t)lane; i < total; i += 64) {
            const uint32_t  row = i / wd, d = i - row * wd;
            const uint32_t  p = T.c0 + 4u * d, j = p >> 6, sh = p & 63u;
            const uint64_t *rw = box + (uint64_t)row * T.pitch;
            uint64_t v = rw[j] >> sh;
            if (sh > 60u && j + 1u < T.pitch) v |= rw[j + 1u] << (64u - sh);        // (the four bits straddle two words)
            uint32_t b = (uint32_t)v & 0xFu;
            const uint32_t left = T.w - 4u * d;                                     // (columns past the run: another run's, or none)
            if (left < 4u) b &= (1u << left) - 1u;
            const uint32_t ones = (b & 1u) | (b & 2u) << 7 | (b & 4u) << 14 | (b & 8u) << 21;
            *reinterpret_cast<uint32_t *>(out + (size_t)row * stride + 4u * d) = ~(ones * 0xFFu);
        }
    }
}

void launch_line_foot(hipStream_t s, const FootJob *jobs, int n_jobs, const FootLine *lines, const TextMapCand *members, const uint16_t *tabs,
                      const uint32_t *bits, uint64_t *feet, FootStat *stat)
{
    if (n_jobs <= 0) return;
    const dim3 grid((unsigned)((n_jobs + FOOT_THREADS / 64 - 1) / (FOOT_THREADS / 64)));
    hipLaunchKernelGGL(k_line_foot, grid, dim3(FOOT_THREADS), 0, s, jobs, n_jobs, lines, members, tabs, bits, feet, stat);
}

void launch_foot_pairs(hipStream_t s, const FootLine *lines, int n_lines, const uint32_t *list, const uint64_t *feet, FootHead *head, FootPair *out,
                       uint32_t cap)
{
    if (n_lines <= 1) return;
    const dim3 grid((unsigned)std::min((n_lines + FOOT_THREADS / 64 - 1) / (FOOT_THREADS / 64), 1 << 16));
    hipLaunchKernelGGL(k_foot_pairs, grid, dim3(FOOT_THREADS), 0, s, lines, n_lines, list, feet, head, out, cap);
}

void launch_foot_links(hipStream_t s, const FootLine *lines, int n_lines, const FootRange *range, const uint32_t *list, const uint64_t *feet, FootHead *head,
                       FootPair *out, uint32_t cap)
{
    if (n_lines <= 1) return;
    const dim3 grid((unsigned)std::min((n_lines + FOOT_THREADS / 64 - 1) / (FOOT_THREADS / 64), 1 << 16));
    hipLaunchKernelGGL(k_foot_links, grid, dim3(FOOT_THREADS), 0, s, lines, n_lines, range, list, feet, head, out, cap);
}

void launch_foot_geom(hipStream_t s, const FootLine *lines, int n_lines, const GeomSlot *slots, const uint64_t *feet, uint64_t *scratch, GeomRec *recs,
                      int32_t *xy)
{
    if (n_lines <= 0) return;
    const dim3 grid((unsigned)std::min(n_lines, 1 << 16));
    hipLaunchKernelGGL(k_foot_geom, grid, dim3(GEOM_THREADS), 0, s, lines, n_lines, slots, feet, scratch, recs, xy);
}

void launch_foot_words(hipStream_t s, const FootLine *lines, int n_lines, const WordsSlot *slots, const uint64_t *feet, WordsRec *recs, WordsRun *runs)
{
    if (n_lines <= 0) return;
    const dim3 grid((unsigned)std::min(n_lines, 1 << 16));
    hipLaunchKernelGGL(k_foot_words, grid, dim3(WORDS_THREADS), 0, s, lines, n_lines, slots, feet, recs, runs);
}

void launch_run_tiles(hipStream_t s, const RunTile *tiles, int n_tiles, const uint64_t *feet, uint8_t *atlas, uint32_t stride)
{
    if (n_tiles <= 0) return;
    const dim3 grid((unsigned)std::min((n_tiles + TILES_THREADS / 64 - 1) / (TILES_THREADS / 64), 1 << 16));
    hipLaunchKernelGGL(k_run_tiles, grid, dim3(TILES_THREADS), 0, s, tiles, n_tiles, feet, atlas, stride);
}
