// resize_tile_body.inl -- the body of k_resize and k_resize_list (er_planes.inl), included into each of them: one 256 x RESIZE_ROWS tile of
// a plane.  In scope where it is included: s_src (LDS), g (ResizeGeom, uniform), s / d (the plane's first source / destination pixel), sstride,
// dstride, tx0, dx0, dy0, active.  Text, not a function: k_resize keeps the code it had before the list kernel shared it.
    if (g.mode != 2) {      // copy / exact 2x2: no tables
        if (!active) return;
        for (int r = 0; r < RESIZE_ROWS && dy0 + r < g.dh; ++r)
            for (int k = 0; k < 4 && dx0 + k < g.dw; ++k)
                d[(size_t)(dy0 + r) * dstride + dx0 + k] = (uint8_t)resize_px(g, s, sstride, 0, dx0 + k, dy0 + r);
        return;
    }
    int sx[4], sx1[4], a0[4], a1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float fx = (float)((min(dx0 + k, g.dw - 1) + 0.5) * g.scale_x - 0.5);
        int   x = (int)floorf(fx);
        fx -= (float)x;
        if (x < 0) { fx = 0.f; x = 0; }
        if (x >= g.sw - 1) { fx = 0.f; x = g.sw - 1; }
        sx[k] = x; sx1[k] = (x + 1 < g.sw) ? x + 1 : x;
        a0[k] = __float2int_rn((1.f - fx) * 2048.f); a1[k] = __float2int_rn(fx * 2048.f);
    }
    // the rows' coefficients are the same for every lane: lane r works out those of row r (the f64 / f32 part of cv::resize's tables) once -- all 64 lanes,
    // before the lanes beyond the plane's last column leave -- and the row loop reads them into scalar registers: as every lane computing every row's they
    // were a sixth of the kernel's vector instructions
    int row_sy, row_b0, row_b1;
    {
        const int dy = dy0 + (int)(threadIdx.x & (RESIZE_ROWS - 1));
        float fy = (float)((dy + 0.5) * g.scale_y - 0.5);
        row_sy = (int)floorf(fy);
        fy -= (float)row_sy;
        row_b0 = __float2int_rn((1.f - fy) * 2048.f); row_b1 = __float2int_rn(fy * 2048.f);
    }
    static_assert((RESIZE_ROWS & (RESIZE_ROWS - 1)) == 0 && RESIZE_ROWS <= 64, "a lane per row of the tile");
    // source window of the tile (uniform over the wave)
    const int x_lo = resize_sx(g, tx0) & ~3;
    const int x_last = resize_sx(g, min(tx0 + 255, g.dw - 1));
    const int x_hi = (x_last + 1 < g.sw) ? x_last + 1 : x_last;
    const int y_lo = min(max(resize_sy(g, dy0), 0), g.sh - 1);
    const int y_hi = min(max(resize_sy(g, min(dy0 + RESIZE_ROWS - 1, g.dh - 1)) + 1, 0), g.sh - 1);
    const int nwords = (x_hi - x_lo) / 4 + 1, nrows = y_hi - y_lo + 1;
    const bool staged = nwords <= RS_WORDS && nrows <= RS_ROWS && (sstride & 3) == 0 && (reinterpret_cast<uintptr_t>(s) & 3) == 0;
    if (staged) {
        // a lane fetches words lane and lane + 64 of every row: all loads of the window (up to 32 per lane) are issued before the first one is
        // waited for -- a loop of load / wait / write pays the memory latency once per round, and that, not arithmetic, was the kernel's time
        static_assert(RS_WORDS <= 128, "two words per lane and row");
        uint32_t v[RS_ROWS][2];
        const uint8_t *src0 = s + (size_t)y_lo * sstride + x_lo + 4 * (int)threadIdx.x;
#pragma unroll
        for (int r = 0; r < RS_ROWS; ++r) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                v[r][j] = 0;
                if (r < nrows && (int)threadIdx.x + 64 * j < nwords) v[r][j] = *reinterpret_cast<const uint32_t *>(src0 + (size_t)r * sstride + 256 * j);
            }
        }
#pragma unroll
        for (int r = 0; r < RS_ROWS; ++r) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (r < nrows && (int)threadIdx.x + 64 * j < nwords && (int)threadIdx.x + 64 * j < RS_WORDS) s_src[r * RS_WORDS + threadIdx.x + 64 * j] = v[r][j];
        }
        __syncthreads();
    }
    const uint8_t *lds = reinterpret_cast<const uint8_t *>(s_src);
    const bool full = dx0 + 4 <= g.dw && (dstride & 3) == 0;
    // (the lanes beyond the plane's last column stay for the form below -- their stores are masked, their taps clamped into the window: the row loop reads
    // the coefficients of row r from lane r, and a lane that had left could not be relied on to hold them)
    if (!(staged && g.scale_x <= 1.5) && !active) return;
    if (staged && g.scale_x <= 1.5) {
        // The taps of the lane's 4 columns lie within 7 source bytes (reduction <= 1.5): per SOURCE row the lane reads the three dwords
        // that hold them, shifts them to its first tap (two v_alignbyte) and picks the 4 left and the 4 right taps with two byte
        // permutes whose selectors are fixed for the tile; the horizontal sums of a source row are kept for the next output row, which
        // mostly needs it again.  A third of the LDS reads of the form below (the byte reads bound this kernel: a byte read costs the
        // LDS what a dword read costs), same arithmetic, same result.
        const int      base = sx[0] & ~3, s0 = sx[0] - base;
        const uint32_t selL = (uint32_t)(sx[0] - sx[0]) | (uint32_t)(sx[1] - sx[0]) << 8 | (uint32_t)(sx[2] - sx[0]) << 16 | (uint32_t)(sx[3] - sx[0]) << 24;
        const uint32_t selR = (uint32_t)(sx1[0] - sx[0]) | (uint32_t)(sx1[1] - sx[0]) << 8 | (uint32_t)(sx1[2] - sx[0]) << 16 | (uint32_t)(sx1[3] - sx[0]) << 24;
        const uint32_t *col = s_src + (base - x_lo) / 4;
        auto hrow = [&](int y, int (&h)[4]) {           // horizontal pass of source row y for the lane's 4 columns
            const uint32_t *p = col + (y - y_lo) * RS_WORDS;
            const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];
            const uint32_t lo = __builtin_amdgcn_alignbyte(d1, d0, (uint32_t)s0), hi = __builtin_amdgcn_alignbyte(d2, d1, (uint32_t)s0);
            const uint32_t L = __builtin_amdgcn_perm(hi, lo, selL), R = __builtin_amdgcn_perm(hi, lo, selR);
#pragma unroll
            for (int k = 0; k < 4; ++k) h[k] = (int)(__umul24((L >> (8 * k)) & 0xFFu, (uint32_t)a0[k]) + __umul24((R >> (8 * k)) & 0xFFu, (uint32_t)a1[k]));
        };
        int ca = -1, cb = -1;               // source rows whose sums are in hA / hB (rows are >= 0)
        int hA[4] = {0, 0, 0, 0}, hB[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (int r = 0; r < RESIZE_ROWS; ++r) {
            const int dy = dy0 + r;
            if (dy >= g.dh) break;
            const int sy = __builtin_amdgcn_readlane(row_sy, r), b0 = __builtin_amdgcn_readlane(row_b0, r), b1 = __builtin_amdgcn_readlane(row_b1, r);
            const int ya = min(max(sy, 0), g.sh - 1), yb = min(max(sy + 1, 0), g.sh - 1);
            // (ya, yb are the same for every lane: uniform branches)
            if (ya == cb) {
#pragma unroll
                for (int k = 0; k < 4; ++k) hA[k] = hB[k];
                ca = cb;
            } else if (ya != ca) { hrow(ya, hA); ca = ya; }
            if (yb == ca) {
#pragma unroll
                for (int k = 0; k < 4; ++k) hB[k] = hA[k];
                cb = yb;
            } else if (yb != cb) { hrow(yb, hB); cb = yb; }
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int o = min((int)(((__umul24((uint32_t)b0, (uint32_t)hA[k] >> 4) >> 16) + (__umul24((uint32_t)b1, (uint32_t)hB[k] >> 4) >> 16) + 2u) >> 2), 255);
                v |= (uint32_t)o << (8 * k);
            }
            uint8_t *o = d + (size_t)dy * dstride + dx0;
            if (full) *reinterpret_cast<uint32_t *>(o) = v;
            else for (int k = 0; k < 4 && dx0 + k < g.dw; ++k) o[k] = (uint8_t)(v >> (8 * k));
        }
        return;
    }
#pragma unroll 4
    for (int r = 0; r < RESIZE_ROWS; ++r) {
        const int dy = min(dy0 + r, g.dh - 1);
        const bool live = dy0 + r < g.dh;
        float fy = (float)((dy + 0.5) * g.scale_y - 0.5);
        int   sy = (int)floorf(fy);
        fy -= (float)sy;
        const int b0 = __float2int_rn((1.f - fy) * 2048.f), b1 = __float2int_rn(fy * 2048.f);
        const int ya = min(max(sy, 0), g.sh - 1), yb = min(max(sy + 1, 0), g.sh - 1);
        uint32_t v = 0;
        if (staged) {
            const uint8_t *p0 = lds + (ya - y_lo) * (RS_WORDS * 4) - x_lo, *p1 = lds + (yb - y_lo) * (RS_WORDS * 4) - x_lo;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t r0 = __umul24(p0[sx[k]], (uint32_t)a0[k]) + __umul24(p0[sx1[k]], (uint32_t)a1[k]);
                const uint32_t r1 = __umul24(p1[sx[k]], (uint32_t)a0[k]) + __umul24(p1[sx1[k]], (uint32_t)a1[k]);
                const int o = min((int)(((__umul24((uint32_t)b0, r0 >> 4) >> 16) + (__umul24((uint32_t)b1, r1 >> 4) >> 16) + 2u) >> 2), 255);
                v |= (uint32_t)o << (8 * k);
            }
        } else {
            const uint8_t *p0 = s + (size_t)ya * sstride, *p1 = s + (size_t)yb * sstride;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t r0 = __umul24(p0[sx[k]], (uint32_t)a0[k]) + __umul24(p0[sx1[k]], (uint32_t)a1[k]);
                const uint32_t r1 = __umul24(p1[sx[k]], (uint32_t)a0[k]) + __umul24(p1[sx1[k]], (uint32_t)a1[k]);
                const int o = min((int)(((__umul24((uint32_t)b0, r0 >> 4) >> 16) + (__umul24((uint32_t)b1, r1 >> 4) >> 16) + 2u) >> 2), 255);
                v |= (uint32_t)o << (8 * k);
            }
        }
        uint8_t *o = d + (size_t)dy * dstride + dx0;
        if (!live) continue;
        if (full) *reinterpret_cast<uint32_t *>(o) = v;
        else for (int k = 0; k < 4 && dx0 + k < g.dw; ++k) o[k] = (uint8_t)(v >> (8 * k));
    }
