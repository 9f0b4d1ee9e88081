// la_gemm_pp_kernel_body.h -- the program of the 256 x 256 GEMM kernel: the text between the braces of gemm_pp_kernel and of
// gemm_pp_kernel_cp (la_gemm_pp_kernel.h), which include it with their template parameters OUT_F32, DUO, T16, LNM and the cache policy CP
// (la_gemm_params.h PPCP_*; gemm_pp_kernel: the constant 0) in scope.  One text, two kernels: the default kernel's code stays what it
// was to the instruction, which a shared function, inlined, did not give (a register more in one instantiation).  No include guard.
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
#ifdef LA_TILE_STAMPS
    const unsigned long long stamp_t0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long stamp_t1 = stamp_t0;
#endif
    const int nwg = p.tiles_m * p.tiles_n;
    const int tile = xcd_remap(blockIdx.x, nwg);
    const TileCoord tc = tile_coord_mb(tile, p.tiles_m, p.tiles_n, p.group, p.mblock);
    const int m0 = tc.tm * PP::TM, n0 = tc.tn * PP::TN;
    const int z = blockIdx.y;
    const T16 *A = reinterpret_cast<const T16 *>(p.A) + (int64_t)z * p.strideA;
    const T16 *W = reinterpret_cast<const T16 *>(p.W) + (int64_t)z * p.strideW;
    const float *bias = p.bias ? p.bias + (int64_t)z * p.strideBias : nullptr;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 2, wc = wave & 3;
    const bool has_bias = (p.epilogue & LA_EPI_BIAS) && bias;
    // Per-column epilogue operands are requested BEFORE the main loop, one column per lane (this wave's 64 columns), and
    // handed to the row-major epilogue layout with ds_bpermute afterwards: all eight waves reach the epilogue together, so a load
    // issued there is a fully exposed L2 round trip per tile.
    const int ncol = min(n0 + wc * 64 + lane, p.N - 1);
    const float bias_l = has_bias ? bias[ncol] : 0.f;
    float csum_l = 0.f;
    if constexpr (LNM == 2 || LNM == 4 || LNM == 6) csum_l = p.ln_csum[ncol];
    // LNM == 2: the tile's 256 row statistics are requested here too (32 rows per wave) and handed to the epilogue through LDS after
    // the main loop: loaded inside the epilogue they were one exposed L2 round trip per pass of 32 rows, four per tile.
    float2 st_pre = make_float2(0.f, 1.f);
    if constexpr (LNM == 2) {
        if (lane < 32) st_pre = reinterpret_cast<const float2 *>(p.ln_stats)[min(m0 + wr * 128 + wc * 32 + lane, p.M - 1)];
    }
    if constexpr (LNM == 6) {                                                 // f16x2 products: (0, row scale) in the statistics' place
        if (lane < 32) st_pre = make_float2(0.f, p.ln_stats[min(m0 + wr * 128 + wc * 32 + lane, p.M - 1)]);
    }

    f32x4 acc[8][4];
#ifdef LA_TILE_STAMPS
#define LA_STAMP_ARG , stamp_t1
#else
#define LA_STAMP_ARG
#endif
    float sacc[4] = {0.f, 0.f, 0.f, 0.f};
    float2 *stats_tab = reinterpret_cast<float2 *>(lds + 120 * 1024);        // LNM == 4: inside ring slot 3, clear of the epilogue staging
    if constexpr (LNM == 4) {
        static_assert(DUO || LNM != 4, "the main loop takes the row statistics only in its hand-placed form");
        const int wc_u = __builtin_amdgcn_readfirstlane(wc);
        switch (wc_u) {                                                       // (the fragment registers are named at compile time)
            case 0: mainloop_duo_asm<T16, 0>(A, p.lda, p.M, W, p.ldw, p.N, p.K, m0, n0, lds, acc LA_STAMP_ARG, sacc); break;
            case 1: mainloop_duo_asm<T16, 1>(A, p.lda, p.M, W, p.ldw, p.N, p.K, m0, n0, lds, acc LA_STAMP_ARG, sacc); break;
            case 2: mainloop_duo_asm<T16, 2>(A, p.lda, p.M, W, p.ldw, p.N, p.K, m0, n0, lds, acc LA_STAMP_ARG, sacc); break;
            default: mainloop_duo_asm<T16, 3>(A, p.lda, p.M, W, p.ldw, p.N, p.K, m0, n0, lds, acc LA_STAMP_ARG, sacc); break;
        }
        // sum over the four lanes that hold one row's four k chunks, then (mean, rstd) of rows wr * 128 + (2 wc + i) * 16 + r
        const float inv_k = 1.0f / (float)p.K;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float s1 = sacc[2 * i], s2 = sacc[2 * i + 1];
            s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16);
            s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
            const float mean = s1 * inv_k;
            const float var = fmaxf(fmaf(-mean, mean, s2 * inv_k), 0.f);
            if (lane < 16) stats_tab[wr * 128 + (2 * wc + i) * 16 + lane] = make_float2(mean, 1.0f / sqrtf(var + 1e-5f));
        }
    } else if constexpr (LNM == 6) {
        static_assert(DUO || LNM != 6, "the segmented-K loop is the hand-placed one");
        mainloop_duo_seg_asm<T16>(A, p.lda, p.M, W, p.ldw, p.N, p.K, p.plane_a, p.plane_w, m0, n0, lds, acc);
    } else if constexpr (DUO && (CP & PPCP_GEMM_A) != 0) {
        // waves 4-7 carry the A image (duo_setup), whose row panels are read by the column tiles of one row block and never again: their
        // copy of the stream has nt in its LDS-DMA pieces, the W waves run the stream as it is (a wave-uniform branch AROUND the loop)
        if (__builtin_amdgcn_readfirstlane(wave) >= 4) mainloop_duo_asm<T16, -1, la::CP_NT>(A, p.lda, p.M, W, p.ldw, p.N, p.K, m0, n0, lds, acc LA_STAMP_ARG);
        else mainloop_duo_asm<T16>(A, p.lda, p.M, W, p.ldw, p.N, p.K, m0, n0, lds, acc LA_STAMP_ARG);
    } else if constexpr (DUO) {
        mainloop_duo_asm<T16>(A, p.lda, p.M, W, p.ldw, p.N, p.K, m0, n0, lds, acc LA_STAMP_ARG);
    } else {
        mainloop_pp<T16>(A, p.lda, p.M, W, p.ldw, p.N, p.K, m0, n0, lds, acc);
    }
    if constexpr (LNM == 2 || LNM == 6) {
        if (lane < 32) stats_tab[wr * 128 + wc * 32 + lane] = st_pre;       // (both main loops end behind a barrier: slot 3 is free)
    }
#ifdef LA_TILE_STAMPS
    const unsigned long long stamp_t2 = __builtin_amdgcn_s_memrealtime();
#endif

    __syncthreads();
    if constexpr (LNM == 3) {
        constexpr int PST = (CP & PPCP_SPLIT_ST) ? la::CP_NT : 0, PLD = (CP & PPCP_SPLIT_LD) ? la::CP_NT : 0;
        // 16-row passes with the residual rows requested one pass ahead (default), or the 32-row passes (LA_EPI_SPLIT_PASS=32: A/B)
        if (p.epilogue & LA_EPI_SPLIT_PASS32) wave_epilogue_split<T16, 0, PST, PLD>(p, z, acc, m0 + wr * 128, n0 + wc * 64, has_bias, bias_l, lds + wave * (32 * EPI_PITCH));
        else wave_epilogue_split<T16, 1, PST, PLD>(p, z, acc, m0 + wr * 128, n0 + wc * 64, has_bias, bias_l, lds + wave * (32 * EPI_PITCH), lds + wave * (32 * EPI_PITCH));
    } else wave_epilogue<OUT_F32, T16, LNM == 2 ? 4 : LNM, 0, CP & PPCP_EPI16_MASK>(p, z, acc, m0 + wr * 128, n0 + wc * 64, has_bias, bias_l, csum_l, lds + wave * (32 * EPI_PITCH), stats_tab, m0);
#ifdef LA_TILE_STAMPS
    if (threadIdx.x == 0 && g_tile_stamps) {
        unsigned long long *o = g_tile_stamps + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8;
        o[0] = stamp_t0; o[1] = stamp_t1; o[2] = stamp_t2; o[3] = __builtin_amdgcn_s_memrealtime();
        unsigned hw_id, xcc_id;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
        o[4] = hw_id; o[5] = xcc_id;
        o[6] = tile;
    }
#endif
