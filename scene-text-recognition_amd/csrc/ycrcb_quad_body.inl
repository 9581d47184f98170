// ycrcb_quad_body.inl -- the body of k_bgr_to_ycrcb and k_bgr_to_ycrcb_list (er_planes.inl), included into each of them: the 4 pixels
// x .. x + 3 of a row (x < w).  In scope where it is included: src (BGR pixel x), yp / crp / cbp (the three planes), dof (pixel x's offset
// in them), x, w, aligned.  Text, not a function: k_bgr_to_ycrcb keeps the code it had before the list kernel shared it.
    if (aligned && x + 4 <= w) {
        const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src);
        const uint32_t wd[3] = {s32[0], s32[1], s32[2]};
        // bytes: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
        int Y[4], Cr[4], Cb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i0 = 3 * k, i1 = 3 * k + 1, i2 = 3 * k + 2;
            const int B = (int)((wd[i0 >> 2] >> (8 * (i0 & 3))) & 255u);
            const int G = (int)((wd[i1 >> 2] >> (8 * (i1 & 3))) & 255u);
            const int R = (int)((wd[i2 >> 2] >> (8 * (i2 & 3))) & 255u);
            ycrcb_px(B, G, R, Y[k], Cr[k], Cb[k]);
        }
        *reinterpret_cast<uint32_t *>(yp + dof)  = Y[0] | (Y[1] << 8) | (Y[2] << 16) | (Y[3] << 24);
        *reinterpret_cast<uint32_t *>(crp + dof) = Cr[0] | (Cr[1] << 8) | (Cr[2] << 16) | (Cr[3] << 24);
        *reinterpret_cast<uint32_t *>(cbp + dof) = Cb[0] | (Cb[1] << 8) | (Cb[2] << 16) | (Cb[3] << 24);
    } else {
        for (int k = 0; k < 4 && x + k < w; ++k) {
            int Y, Cr, Cb;
            ycrcb_px(src[3 * k], src[3 * k + 1], src[3 * k + 2], Y, Cr, Cb);
            yp[dof + k] = (uint8_t)Y; crp[dof + k] = (uint8_t)Cr; cbp[dof + k] = (uint8_t)Cb;
        }
    }
