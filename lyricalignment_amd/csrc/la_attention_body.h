// la_attention_body.h -- the program of the 16-bit attention kernel: the text between the braces of attention_bf16_kernel and of
// attention_bf16_kernel_cp (la_attention.hip), which include it with their template parameters T16, NW, FOLD and the cache policy CP
// (attention_bf16_kernel: the constant 0) in scope.  One text, two kernels: the default kernel's code stays what it was to the instruction.
// No include guard.
    constexpr int KO = LA_ATTN_KO;
    constexpr int POL_QO = (CP & 1) ? la::CP_NT : 0, POL_KV = (CP & 2) ? la::CP_NT : 0;
    constexpr int QT = 32 * NW, PER = 8 / NW;
    typedef Half16<T16> HT;
    typedef typename HT::vec8 vec8;
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * 2 * IMG];  // [buf][K|V][64][128 B] = 32 KiB
    const int T = p.kv_len;
    const BlockCoord bc = block_coord((p.q_len + QT - 1) / QT, p.n_head, p.batch);
    const int qt = bc.qt, head = bc.head, clip = bc.clip;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i32 = lane & 31, h = lane >> 5;
    // (pointer arithmetic in 16-bit elements; bf16_t stands for either storage type here)
    const bf16_t *base = reinterpret_cast<const bf16_t *>(p.q) + (int64_t)clip * p.q_bs * p.ld_q + head * 64;
    const unsigned short *kbase = reinterpret_cast<const unsigned short *>(p.k) + (int64_t)clip * p.kv_bs * p.ld_kv + head * 64;
    const unsigned short *vbase = reinterpret_cast<const unsigned short *>(p.v) + (int64_t)clip * p.kv_bs * p.ld_kv + head * 64;

    // Q fragments (B operand): lane (q = i32, h) holds Q[q][16c + 8h .. +8], c = 0..3
    int qrow = qt * QT + wave * 32 + i32;
    const bool q_valid = qrow < p.q_len;
    qrow = q_valid ? qrow : p.q_len - 1;
    uint4 qf[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        // (policy 0 keeps its statement as it was written: the default kernel's code is the same to the instruction)
        if constexpr (POL_QO == 0) qf[c] = *reinterpret_cast<const uint4 *>(base + (int64_t)qrow * p.ld_q + 16 * c + 8 * h);
        else qf[c] = la::load_pol<POL_QO, uint4>(base + (int64_t)qrow * p.ld_q + 16 * c + 8 * h);
    }

    f32x16 o[2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[b][r] = 0.f;
    float m_run = FOLD ? 0.f : -INFINITY, l_part = 0.f;
    int plain = FOLD ? 1 : 0;               // FOLD: no query of this wave has needed a maximum yet: P = exp2(s) as it stands (wave-uniform)
    const float kScale = FOLD ? 1.0f : p.score_scale;

    int nkv = (T + KT - 1) / KT;
    const int nkv_all = nkv;
    if (p.causal) nkv = min(nkv, (min(p.q_len, (qt + 1) * QT) - 1) / KT + 1);   // tiles above the block's diagonal are all masked
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(la::lds_addr_u32(lds));
    const KvOff<PER> off_full = kv_offsets<PER, 2>(p.ld_kv, 0, KT, wave, lane);                      // every row valid
    const KvOff<PER> off_last = kv_offsets<PER, 2>(p.ld_kv, (nkv_all - 1) * KT, T, wave, lane);      // rows clamped to key T-1
    auto stage = [&](int t, unsigned buf) __attribute__((always_inline)) {
        const KvOff<PER> &off = t == nkv_all - 1 ? off_last : off_full;
        // (both sources before the first load, K and V pieces alternating: the order this loop's scalar work was compiled in)
        const unsigned short *ks = kbase + (int64_t)(t * KT) * p.ld_kv, *vs = vbase + (int64_t)(t * KT) * p.ld_kv;
        stage_pair<PER, POL_KV>(ks, off.k, buf, vs, 0, off.v, buf + IMG, wave);
    };
    stage(0, lds0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int c = 0; c < 4; ++c) pin_frags(qf[c]);
    __syncthreads();

    const int g = lane >> 4, q4 = (lane & 15) >> 2, pp = lane & 3;

    auto tile = [&](int t, auto curc) __attribute__((always_inline)) {
        constexpr int cur = decltype(curc)::value;
        const unsigned char *kl = lds + cur * 2 * IMG;
        const unsigned char *vl = kl + IMG;
        if (t + 1 < nkv && !(KO & 8)) stage(t + 1, lds0 + (cur ^ 1) * 2 * IMG);
        // ---- S^T = K Q^T : two 32-key sub-tiles ----
        // all eight K fragments are requested before the first MFMA (32 VGPRs; the kernel has room): the reads return under
        // the MFMAs instead of one ds_read -> wait -> MFMA round trip per fragment
        f32x16 s[2];
        typedef std::integral_constant<int, 0> Sub0;
        typedef std::integral_constant<int, 1> Sub1;
        typedef std::integral_constant<int, 2> SubBoth;
        // scores of sub-tile `which` (2 = both).  serial: the redo path -- one fragment pair in flight (few live registers)
        auto scores = [&](auto serialc, auto whichc) {
            constexpr bool serial = decltype(serialc)::value;
            constexpr int lo = decltype(whichc)::value == 2 ? 0 : decltype(whichc)::value;
            constexpr int hi = decltype(whichc)::value == 2 ? 2 : lo + 1;
            uint4 kf[2][4];
#pragma unroll
            for (int sub = lo; sub < hi; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) s[sub][r] = 0.f;
            if constexpr (!serial) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int sub = lo; sub < hi; ++sub) {
                        if constexpr (KO & 4) kf[sub][c] = qf[(c + sub) & 3];
                        else kf[sub][c] = row_frag<uint4>(kl, sub * 32 + i32, c, h);
                    }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if constexpr (serial) {
#pragma unroll
                    for (int sub = lo; sub < hi; ++sub) kf[sub][c] = row_frag<uint4>(kl, sub * 32 + i32, c, h);
                }
#pragma unroll
                for (int sub = lo; sub < hi; ++sub)
                    if constexpr (KO & 16) s[sub][c] += __builtin_bit_cast(float, kf[sub][c].x) + __builtin_bit_cast(float, kf[sub][c].w);
                    else s[sub] = HT::mfma32(__builtin_bit_cast(vec8, kf[sub][c]), __builtin_bit_cast(vec8, qf[c]), s[sub]);
                if constexpr (serial) __builtin_amdgcn_sched_barrier(0);
            }
            // ---- mask keys >= kv_len (last tile) and, for the causal decoder self-attention, keys after the query ----
            if ((t + 1) * KT > T || p.causal) {
                const int kmax = p.causal ? min(T - 1, qrow) : T - 1;
#pragma unroll
                for (int sub = lo; sub < hi; ++sub)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (t * KT + sub * 32 + acc_row(r, h) > kmax) s[sub][r] = -INFINITY;
            }
        };
        // s <- exp2(s log2 e - m), returns this lane's partial row sum
        // (two at a time: v_pk_fma_f32 / v_pk_add_f32, 16 + 16 instructions instead of 32 + 32)
        auto exponentials = [&](float m, auto whichc) -> float {
            constexpr int lo = decltype(whichc)::value == 2 ? 0 : decltype(whichc)::value;
            constexpr int hi = decltype(whichc)::value == 2 ? 2 : lo + 1;
            // plain v_fma_f32 / v_add_f32, two independent partial sums -- NOT packed f32: v_pk_fma_f32 / v_pk_add_f32 / v_pk_mul_f32
            // do not run beside the matrix pipe at all (tools/valu_mfma_overlap.hip: 0 % of a block of them hides under MFMAs,
            // 45-70 % of any other vector instruction does) and cost 1.8x a plain instruction for 2x the work; measured here:
            // 344 us plain against 349 us packed
            float ps0 = 0.f, ps1 = 0.f;
            auto body = [&](auto subtract_m) {
#pragma unroll
                for (int sub = lo; sub < hi; ++sub)
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        float a0, a1;
                        if constexpr (FOLD) {
                            a0 = s[sub][r]; a1 = s[sub][r + 1];
                            if constexpr (decltype(subtract_m)::value) { a0 -= m; a1 -= m; }
                        } else { a0 = fmaf(s[sub][r], kScale, -m); a1 = fmaf(s[sub][r + 1], kScale, -m); }
                        const float p0 = (KO & 1) ? a0 : __builtin_amdgcn_exp2f(a0), p1 = (KO & 1) ? a1 : __builtin_amdgcn_exp2f(a1);
                        s[sub][r] = p0;
                        s[sub][r + 1] = p1;
                        ps0 += p0;
                        ps1 += p1;
                    }
            };
            if (FOLD && plain) body(std::false_type{});      // wave-uniform (an SGPR): only the redo path clears it
            else body(std::true_type{});
            return ps0 + ps1;
        };
        auto tile_max = [&](auto whichc) -> float {
            constexpr int lo = decltype(whichc)::value == 2 ? 0 : decltype(whichc)::value;
            constexpr int hi = decltype(whichc)::value == 2 ? 2 : lo + 1;
            float mx = -INFINITY;
#pragma unroll
            for (int sub = lo; sub < hi; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[sub][r]);
            return fmaxf(mx, __shfl_xor(mx, 32)) * kScale;
        };
        auto rescale = [&](float alpha) {
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[b][r] *= alpha;
        };
        // ---- O^T += V^T P^T for one 32-key sub-tile ----
        auto pv_sub = [&](auto subc) {
            constexpr int sub = decltype(subc)::value;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                vec8 pf;  // element j <-> accumulator register 8*ks + j <-> key sub*32 + 16ks + 8(j>>2) + 4h + (j&3)
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[j] = (typename HT::elem)s[sub][8 * ks + j];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    s16x8 vf;
                    if constexpr (KO & 2) vf = __builtin_bit_cast(s16x8, qf[(2 * sub + ks + b) & 3]);
                    else {
                        // (tr_frag's text, inline: as a call the compiler forms the row index with one instruction fewer before the loop,
                        // and this site keeps the parent's instruction sequence)
                        const int key0 = sub * 32 + 16 * ks + 4 * (g >> 1);
                        const int slot = b * 4 + 2 * (g & 1) + (pp >> 1);
                        const int r0 = key0 + q4, r1 = key0 + 8 + q4;
                        typedef __attribute__((address_space(3))) s16x4 *lds_s16x4;
                        const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(vl + r0 * 128 + ((slot ^ vswz(r0)) << 4) + (pp & 1) * 8));
                        const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(vl + r1 * 128 + ((slot ^ vswz(r1)) << 4) + (pp & 1) * 8));
                        vf = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
                    }
                    if constexpr (KO & 16) o[b][2 * sub + ks] += (float)vf[0] + (float)vf[7] + (float)pf[0] + (float)pf[7];
                    else o[b] = HT::mfma32(__builtin_bit_cast(vec8, vf), pf, o[b]);
                }
            }
        };
        // the textbook step for sub-tile(s) `which`, scores recomputed from the K tile in LDS (the optimistic form's redo path)
        auto redo = [&](auto whichc) -> float {
            scores(std::true_type{}, whichc);
            const float m_new = fmaxf(m_run, tile_max(whichc));
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);    // exp2(-inf) = 0 on the first tile
            m_run = m_new;
            plain = 0;
            rescale(alpha);
            l_part *= alpha;
            return exponentials(m_new, whichc);
        };
        scores(std::false_type{}, SubBoth{});
        // per 32-key sub-tile, so that sub-tile 1's exponentials and sub-tile 0's PV MFMAs share a basic block (hipcc interleaves them)
        float ps0 = exponentials(m_run, Sub0{});
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(!(ps0 <= HT::kPLimit)) != 0, 0)) ps0 = redo(Sub0{});   // wave-uniform, rare
        l_part += ps0;
        float ps1 = exponentials(m_run, Sub1{});
        pv_sub(Sub0{});
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(!(ps1 <= HT::kPLimit)) != 0, 0)) ps1 = redo(Sub1{});
        l_part += ps1;
        pv_sub(Sub1{});
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if constexpr (!(KO & 32)) __syncthreads();
    };
    sweep2(0, nkv, tile);
    if constexpr (FOLD) {
        // a sum outside 2^-100 .. 2^100 (all of a query's scores far below 0, or an overflow the per-tile test did not see):
        // the whole block once more with a maximum from the first tile on (block-uniform decision, said so to the compiler;
        // a second, cold copy of the tile loop rather than a loop around the first: that nest cost 50 VGPRs)
        const float l0 = l_part + __shfl_xor(l_part, 32);
        if (__builtin_amdgcn_readfirstlane(__syncthreads_or(q_valid && !(l0 >= 0x1p-100f && l0 <= 0x1p100f)))) {
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[b][r] = 0.f;
            m_run = -INFINITY; l_part = 0.f; plain = 0;
            stage(0, lds0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            sweep2(0, nkv, tile);
        }
    }

    // ---- epilogue: O[q][dv] = O^T / l ----
    const float l = l_part + __shfl_xor(l_part, 32);
    const float inv = 1.0f / l;
    if (q_valid) {
        bf16_t *orow = reinterpret_cast<bf16_t *>(p.out) + ((int64_t)clip * p.out_bs + qrow) * p.ld_out + head * 64;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                if constexpr (POL_QO == 0)
                    *reinterpret_cast<ushort4 *>(orow + 32 * b + 8 * r4 + 4 * h) =
                        la::Pack4<T16>::run(o[b][4 * r4 + 0] * inv, o[b][4 * r4 + 1] * inv, o[b][4 * r4 + 2] * inv, o[b][4 * r4 + 3] * inv);
                else
                    la::store_pol<POL_QO>(orow + 32 * b + 8 * r4 + 4 * h,
                                          la::Pack4<T16>::run(o[b][4 * r4 + 0] * inv, o[b][4 * r4 + 1] * inv, o[b][4 * r4 + 2] * inv, o[b][4 * r4 + 3] * inv));
            }
    }
