// nv12_quad_body.inl -- the body of k_nv12_to_ycrcb and k_nv12_to_ycrcb_list (er_planes.inl), included into each of them: the 4 pixels
// x .. x + 3 of a row (x < w, x even).  In scope where it is included: ys (luma pixel x), uv (the chroma pair of pixel x: byte x of its
// chroma row), yp / crp / cbp (the three planes), dof (pixel x's offset in them), x, w, aligned.  Text, not a function: k_nv12_to_ycrcb
// keeps the code it had before the list kernel shared it.
    if (aligned && x + 4 <= w) {
        const uint32_t yy = *reinterpret_cast<const uint32_t *>(ys), c = *reinterpret_cast<const uint32_t *>(uv);     // U0 V0 U1 V1
        const uint32_t u0 = c & 0xFFu, v0 = (c >> 8) & 0xFFu, u1 = (c >> 16) & 0xFFu, v1 = c >> 24;
        *reinterpret_cast<uint32_t *>(yp + dof) = yy;
        *reinterpret_cast<uint32_t *>(crp + dof) = v0 * 0x0101u | (v1 * 0x0101u) << 16;
        *reinterpret_cast<uint32_t *>(cbp + dof) = u0 * 0x0101u | (u1 * 0x0101u) << 16;
    } else {
        for (int k = 0; k < 4 && x + k < w; ++k) {
            yp[dof + k] = ys[k];
            cbp[dof + k] = uv[(k & ~1)];
            crp[dof + k] = uv[(k & ~1) + 1];
        }
    }
