// svd_copies_yuv420_body.inc -- the body of svd_copies_yuv420_kernel and svd_copies_soft_yuv420_kernel (planar_copies_kernels.hiph),
// included inside each, as svd_copies_rgb8_body.inc.  The including kernel provides in, out, g, frames, a, k, hist, the constants
// FMT, VERIFY, MULTI, SOFT, and for SOFT shist and sf.
    const int t = threadIdx.x;
    const int tiles = (g.nblk + kThreads - 1) / kThreads;
    int f, bx;
    if (!xcd_tile(0, tiles, frames, f, bx)) return;       // whole workgroup: before any barrier
    const int c = bx * kThreads + t;
    const bool valid = c < g.nblk;
    const bool use_hist = svd_readout_begin((LdsHist)hist, VERIFY, a.counts, a.L);
    bool use_shist = false;
    if constexpr (SOFT) use_shist = svd_readout_begin((LdsHist)shist, true, reinterpret_cast<const int32_t *>(sf.soft), a.L);
    const int cc = valid ? c : g.nblk - 1;
    int bi, bj;
    divmod_small(cc, g.wb, g.inv_wb, bi, bj);
    const uint8_t *frame = in + (size_t)f * g.frame_stride;
    PPair p[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = load_pair<FMT>(frame, g, bi, bj, i);
    // the bit-independent half of svd_update, per marked channel (MULTI: channels 0, 1, 2; else channel 1 only)
    constexpr int NCH = MULTI ? 3 : 1;
    Svd4 sv[NCH];
    {
        float B[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) pair_ll<1>(p[i], B[i]);
        if constexpr (MULTI) {                          // wave-uniform branches: the scales are kernel arguments
            if (a.scales[1] > 0.f) sv[1] = svd4_top(B);
            if (a.scales[0] > 0.f) {
#pragma unroll
                for (int i = 0; i < 4; ++i) pair_ll<0>(p[i], B[i]);
                sv[0] = svd4_top(B);
            }
            if (a.scales[2] > 0.f) {
#pragma unroll
                for (int i = 0; i < 4; ++i) pair_ll<2>(p[i], B[i]);
                sv[2] = svd4_top(B);
            }
        } else {
            sv[0] = svd4_top(B);
        }
    }
#pragma unroll 1
    for (int q = 0; q < k.copies; ++q) {
        // every copy converts its pixels from the planar bytes again: without this the compiler hoists the 64 pixels' RGB out of
        // the copy loop (loop-invariant) and spills them
#pragma unroll
        for (int i = 0; i < 4; ++i) forget(p[i]);
        const int wbit = a.wm[(size_t)copy_row(k, q, f, a.n_wm) * a.N + cc];
        // the gains now, the rank-1 products svd_du() one row pair at a time: 12 floats per copy instead of 48 live ones
        float gu = 0.f, gy = 0.f, gv = 0.f;
        if constexpr (MULTI) {
            if (a.scales[1] > 0.f) gu = svd_gain(sv[1], wbit, a.scales[1]);
            if (a.scales[0] > 0.f) gy = svd_gain(sv[0], wbit, a.scales[0]);
            if (a.scales[2] > 0.f) gv = svd_gain(sv[2], wbit, a.scales[2]);
        } else {
            gu = svd_gain(sv[0], wbit, a.scales[1]);
        }
        uint8_t *oframe = out + (size_t)q * k.out_stride + (size_t)f * g.frame_stride;
        float B[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float dy[4], du[4], dv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (MULTI) {
                    du[j] = a.scales[1] > 0.f ? svd_du(sv[1], gu, i, j) : 0.f;
                    dy[j] = a.scales[0] > 0.f ? svd_du(sv[0], gy, i, j) : 0.f;
                    dv[j] = a.scales[2] > 0.f ? svd_du(sv[2], gv, i, j) : 0.f;
                } else {
                    du[j] = svd_du(sv[0], gu, i, j);
                    dy[j] = 0.f;
                    dv[j] = 0.f;
                }
            }
            PPair o;
            mark_pair<true, MULTI, VERIFY>(p[i], dy, du, dv, o, B[i]);
            if (valid) store_pair<FMT>(oframe, g, bi, bj, i, o);
        }
        if constexpr (SOFT) {
            const bool on = a.scales[1] > 0.f;
            const float s0 = on ? svd4_top_value(B, true) : 0.f;      // the hard verify's value and the stand-alone read-outs'
            if (a.counts != nullptr || a.bits != nullptr) {          // wave-uniform: the hard verify in the same launch
                const int bit = on && fmod_pos(s0, a.scales[1]) > a.scales[1] * 0.5f ? 1 : 0;     // svd_read_bit
                svd_readout_emit<true>((LdsHist)hist, bit, valid, f, c, bx, tiles, a.N, a.L, a.bits ? a.bits + (size_t)q * k.bits_stride : nullptr,
                                       a.counts ? a.counts + (size_t)q * k.counts_stride : nullptr, a.partial, use_hist);
            }
            svd_soft_emit<true>((LdsHist)shist, on ? svd_soft_metric(s0, a.scales[1]) : 0, valid, f, c, a.L, sf.soft + (size_t)q * sf.stride, use_shist);
        } else if constexpr (VERIFY) {
            const int bit = a.scales[1] > 0.f ? svd_read_bit(B, a.scales[1], true) : 0;
            svd_readout_emit<true>((LdsHist)hist, bit, valid, f, c, bx, tiles, a.N, a.L, a.bits ? a.bits + (size_t)q * k.bits_stride : nullptr,
                                   a.counts ? a.counts + (size_t)q * k.counts_stride : nullptr, a.partial, use_hist);
        }
    }
