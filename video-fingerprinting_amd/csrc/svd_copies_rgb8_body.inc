// svd_copies_rgb8_body.inc -- the body of svd_copies_rgb8_kernel and svd_copies_soft_rgb8_kernel (copies_kernels.hiph), included
// inside each: the two kernels are one text.  (As an inline function taking the kernels' arguments the body compiles to different
// instructions for the existing kernel -- the arguments' noalias / kernarg properties do not survive the call -- and that kernel
// keeps its code: profiles/copies_soft_kernel_diff.txt.)  The including kernel provides in, out, g, a, k, hist, the constants
// ALIGNED, VERIFY, MULTI, SOFT, and for SOFT shist and sf.
    const int t = threadIdx.x;
    int f, bx;
    const int tiles = (g.nblk + kThreads - 1) / kThreads;
    if (!xcd_tile(0, tiles, g.frames, f, bx)) return;       // linear order, as svd_rgb8_kernel
    const int c = bx * kThreads + t;
    const bool valid = c < g.nblk;
    const bool use_hist = svd_readout_begin((LdsHist)hist, VERIFY, a.counts, a.L);
    bool use_shist = false;
    if constexpr (SOFT) use_shist = svd_readout_begin((LdsHist)shist, true, reinterpret_cast<const int32_t *>(sf.soft), a.L);
    const int cc = valid ? c : g.nblk - 1;
    int bi, bj;
    divmod_small(cc, g.wb, g.inv_wb, bi, bj);
    const size_t off = (size_t)f * g.frame_stride + ((size_t)bi * 8 * g.W + (size_t)bj * 8) * 3;
    const int pitch = g.W * 3;
    Px8 raw[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) raw[r] = load_px8<ALIGNED>(in + off + (size_t)r * pitch);
    constexpr bool KEEP_S2 = VERIFY && !MULTI;         // channel 2's bytes survive the marking: its 2x2 sums serve every verify
    float s2[KEEP_S2 ? 4 : 1][4];
    // the bit-independent half of svd_update, per marked channel (MULTI: channels 0, 1, 2; else channel 1 only)
    constexpr int NCH = MULTI ? 3 : 1;
    Svd4 sv[NCH];
    {
        float B[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (KEEP_S2) haar_ll_row_px<1, 1>(raw[2 * i], raw[2 * i + 1], B[i], s2[i]);
            else haar_ll_row_px(raw[2 * i], raw[2 * i + 1], B[i]);
        }
        if constexpr (MULTI) {                          // wave-uniform branches: the scales are kernel arguments
            if (a.scales[1] > 0.f) sv[1] = svd4_top(B);
            if (a.scales[0] > 0.f) {
#pragma unroll
                for (int i = 0; i < 4; ++i) haar_ll_row_px<0>(raw[2 * i], raw[2 * i + 1], B[i]);
                sv[0] = svd4_top(B);
            }
            if (a.scales[2] > 0.f) {
#pragma unroll
                for (int i = 0; i < 4; ++i) haar_ll_row_px<2>(raw[2 * i], raw[2 * i + 1], B[i]);
                sv[2] = svd4_top(B);
            }
        } else {
            sv[0] = svd4_top(B);
        }
    }
#pragma unroll 1
    for (int q = 0; q < k.copies; ++q) {
        // every copy decodes its pixels from the raw bytes again: without this the compiler hoists the 64 pixels' Y / U / V out
        // of the copy loop (loop-invariant) and spills them
#pragma unroll
        for (int r = 0; r < 8; ++r) forget(raw[r]);
        const int wbit = a.wm[(size_t)copy_row(k, q, f, a.n_wm) * a.N + cc];
        float dU[4][4], dY[MULTI ? 4 : 1][4], dV[MULTI ? 4 : 1][4];
        if constexpr (MULTI) {
            const float gu = a.scales[1] > 0.f ? svd_gain(sv[1], wbit, a.scales[1]) : 0.f;
            const float gy = a.scales[0] > 0.f ? svd_gain(sv[0], wbit, a.scales[0]) : 0.f;
            const float gv = a.scales[2] > 0.f ? svd_gain(sv[2], wbit, a.scales[2]) : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    dU[i][j] = a.scales[1] > 0.f ? svd_du(sv[1], gu, i, j) : 0.f;
                    dY[i][j] = a.scales[0] > 0.f ? svd_du(sv[0], gy, i, j) : 0.f;
                    dV[i][j] = a.scales[2] > 0.f ? svd_du(sv[2], gv, i, j) : 0.f;
                }
        } else {
            const float gu = svd_gain(sv[0], wbit, a.scales[1]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) dU[i][j] = svd_du(sv[0], gu, i, j);
        }
        uint8_t *dst = out + (size_t)q * k.out_stride + off;
        float B[4][4];
        Px8 oprev;                                     // marked pixels of the even row of a pair (verify)
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const Px8 &px = raw[r];
            Px8 o = px;                                // channel 2 is untouched unless MULTI (see svd_rgb8_kernel)
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const float c0 = px_byte(px, 3 * x), c1 = px_byte(px, 3 * x + 1), c2 = px_byte(px, 3 * x + 2);
                float n0, n1, n2, dy = 0.f, dv = 0.f;
                if constexpr (MULTI) { dy = dY[r >> 1][x >> 1]; dv = dV[r >> 1][x >> 1]; }
                svd_mark_px<MULTI>(c0, c1, c2, dy, dU[r >> 1][x >> 1], dv, n0, n1, n2);
                o.w[(3 * x) >> 2] = put_u8(n0, (3 * x) & 3, o.w[(3 * x) >> 2]);
                o.w[(3 * x + 1) >> 2] = put_u8(n1, (3 * x + 1) & 3, o.w[(3 * x + 1) >> 2]);
                if constexpr (MULTI) o.w[(3 * x + 2) >> 2] = put_u8(n2, (3 * x + 2) & 3, o.w[(3 * x + 2) >> 2]);
            }
            if (valid) store_px8<ALIGNED>(dst + (size_t)r * pitch, o);
            if constexpr (VERIFY) {                    // what the detector will see: the rounded u8 pixels
                if (r & 1) {
                    if constexpr (KEEP_S2) haar_ll_row_px<1, 2>(oprev, o, B[r >> 1], s2[r >> 1]);
                    else haar_ll_row_px(oprev, o, B[r >> 1]);
                }
                else oprev = o;
            }
        }
        if constexpr (SOFT) {
            const bool on = a.scales[1] > 0.f;
            const float s0 = on ? svd4_top_value(B, true) : 0.f;      // the stand-alone read-outs' value
            if (a.counts != nullptr || a.bits != nullptr) {          // wave-uniform: the hard verify in the same launch
                const float sh = a.scales[1] < kLooseReadoutMinScale ? s0 : svd4_top_value(B, false);
                const int bit = on && fmod_pos(sh, a.scales[1]) > a.scales[1] * 0.5f ? 1 : 0;     // svd_read_bit
                svd_readout_emit<true>((LdsHist)hist, bit, valid, f, c, bx, tiles, a.N, a.L, a.bits ? a.bits + (size_t)q * k.bits_stride : nullptr,
                                       a.counts ? a.counts + (size_t)q * k.counts_stride : nullptr, a.partial, use_hist);
            }
            svd_soft_emit<true>((LdsHist)shist, on ? svd_soft_metric(s0, a.scales[1]) : 0, valid, f, c, a.L, sf.soft + (size_t)q * sf.stride, use_shist);
        } else if constexpr (VERIFY) {
            const int bit = a.scales[1] > 0.f ? svd_read_bit(B, a.scales[1], a.scales[1] < kLooseReadoutMinScale) : 0;
            svd_readout_emit<true>((LdsHist)hist, bit, valid, f, c, bx, tiles, a.N, a.L, a.bits ? a.bits + (size_t)q * k.bits_stride : nullptr,
                                   a.counts ? a.counts + (size_t)q * k.counts_stride : nullptr, a.partial, use_hist);
        }
    }
