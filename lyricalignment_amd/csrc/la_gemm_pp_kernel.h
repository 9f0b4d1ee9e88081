// la_gemm_pp_kernel.h -- the 256 x 256 GEMM kernel of the 16-bit modes (every large Linear / conv-as-GEMM of the encoder, the GRU
// input projections) and its launchers, as templates over the operand type: instantiated by la_gemm_pp_bf16.hip and
// la_gemm_pp_f16.hip (two translation units, so the two operand types compile in parallel).
// Main loops: la_gemm_pp.h (hand-placed flat stream / quadrant ping-pong).  Epilogues: la_gemm_epilogue.h.
#pragma once
#include <algorithm>

#include "la_gemm_epilogue.h"

namespace la {
namespace gemm {

#ifdef LA_TILE_STAMPS
// Diagnostic build only (tools/tile_timeline.py): per workgroup (wall clock at entry, after the prologue, after the main loop, at
// the end; HW_ID) into a buffer that nothing else reads -- where a tile's lifetime goes and how long a CU waits for its next one.
static __device__ unsigned long long *g_tile_stamps = nullptr;
static inline int set_tile_stamps_here(void *buf) {
    unsigned long long *b = static_cast<unsigned long long *>(buf);
    return hipMemcpyToSymbol(HIP_SYMBOL(g_tile_stamps), &b, sizeof(b)) == hipSuccess ? LA_OK : LA_EHIP;
}
#endif

// The kernel's program is la_gemm_pp_kernel_body.h.  CP (la_gemm_params.h PPCP_*): the cache policy of its streamed accesses, compiled into
// the instruction text -- gemm_pp_kernel is CP = 0, the instructions as they always were; gemm_pp_kernel_cp carries the other values
// (options cp_epi16, cp_split_st, cp_split_ld, cp_gemm_a), one instantiation per combination, chosen per launch.
template <bool OUT_F32, bool DUO, typename T16, int LNM = 0>
__global__ __launch_bounds__(PP::THREADS, 2) void gemm_pp_kernel(GemmParams p) {
    constexpr int CP = 0;
#include "la_gemm_pp_kernel_body.h"
}
template <bool OUT_F32, bool DUO, typename T16, int LNM, int CP>
__global__ __launch_bounds__(PP::THREADS, 2) void gemm_pp_kernel_cp(GemmParams p) {
    static_assert(CP != 0, "CP = 0 is gemm_pp_kernel");
#include "la_gemm_pp_kernel_body.h"
}

template <bool OUT_F32, bool DUO, typename T16, int LNM = 0, int CP = 0>
int launch_pp_loop(GemmParams p, int batch, hipStream_t stream) {
    void (*kern)(GemmParams);
    if constexpr (CP == 0) kern = gemm_pp_kernel<OUT_F32, DUO, T16, LNM>;
    else kern = gemm_pp_kernel_cp<OUT_F32, DUO, T16, LNM, CP>;
    static la::DeviceOnce attr_once;
    if (attr_once.pending()) {
        LA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, PP::LDS));
        attr_once.mark();
    }
    p.tiles_m = la::cdiv(p.M, PP::TM);
    p.tiles_n = la::cdiv(p.N, PP::TN);
    // column tiles that walk the M dimension together (their W panels share the XCD's L2 with the streaming A panel).
    // At least 4: with fewer, the K=4096 GEMM (N = 4 tiles) re-reads its 2 MB-per-row-block A panel once per column tile
    // (in-pipeline sweep: 1 -> 46.1 ms/step, 4 -> 45.7, 8 -> 45.9, 16 -> 46.4).
    p.group = la::dev_env("LA_GEMM_GROUP") ? std::min(p.group, p.tiles_n) : std::min(p.tiles_n, std::max(4, p.group / 2));
    // More than one column group: the groups follow each other inside blocks of 32 row tiles (tile_coord_mb), so a block's A panels
    // (16 MB at K = 1024) are re-read per group out of the Infinity Cache instead of once per sweep over all of M.  Alone on the chip
    // with cold A the MLP-up shape runs 438 -> 352 us (tools/kbench.py order); inside the pipeline, where A was just written, 0.6 %
    // of the step (profiles/r4_ab_mblock.txt).
    // (the f16x2 form -- LNM 6 -- stages both planes of every operand row: twice the bytes per row panel, and blocks of 8 row tiles measured best there:
    //  QKV 767 -> 749 us, MLP-up 1036 -> 1015 us at 48000 rows, the N = 1024 shapes flat; profiles/r6_x2_tile_order.txt)
    p.mblock = p.tiles_n > p.group ? (LNM == 6 ? 8 : 32) : 0;
    // (experiment build only: developer sweeps / probes, read per launch)
    if (const char *g = la::dev_env("LA_GEMM_MBLOCK")) p.mblock = atoi(g);
    if (const char *g = la::dev_env("LA_GELU_PK")) p.epilogue |= atoi(g) == 2 ? 8192 : 4096;
    if (const char *g = la::dev_env("LA_EPI_PROBE")) p.epilogue |= (atoi(g) & 7) << 16;
    // (LNM 6: the f16x2 form of a float32 product -- its own timer family, counted at its ALGORITHMIC flops: a third of the MFMA work)
    la::TimerScope ts(LNM == 6 ? "gemm_f16x2" : "gemm_bf16", stream, 2.0 * p.M * p.N * p.K * batch);
    hipLaunchKernelGGL(kern, dim3(p.tiles_m * p.tiles_n, batch), dim3(PP::THREADS), PP::LDS, stream, p);
    LA_LAUNCH_CHECK();
    return LA_OK;
}

// Main loop: the hand-placed flat stream (mainloop_duo_asm) where its k-step structure fits -- K a multiple of 128 (four k-steps
// of 32 per ring turn), at least 256 -- else the quadrant ping-pong; option gemm_loop = 99 (LA_PP_DBG) forces the ping-pong
// everywhere.  Same tile, same accumulation order, same epilogue arithmetic: identical bits.
template <bool OUT_F32, typename T16>
int launch_pp(GemmParams p, int batch, hipStream_t stream) {
    const bool duo = p.K % 128 == 0 && p.K >= 256 && la::opts().gemm_loop != 99;
    const int lnm = p.ln_stats ? 2 : (p.ln_csum ? 4 : ((OUT_F32 && p.C2) ? 1 : 0));
#ifdef LA_EXPERIMENTS
    if constexpr (std::is_same<T16, bf16_t>::value) {
        int rc = LA_OK;
        if (lab_try_launch(p, batch, OUT_F32, lnm, duo, stream, &rc)) return rc;
    }
#endif
    if (lnm == 4) {
        la::set_error("gemm_fused_ln: the in-loop row statistics (ln_csum without ln_stats) were measured slower than la_row_stats16 and live "
                      "in the experiment build only (tools/build_variant.sh, bfloat16)");
        return LA_EUNSUPPORTED;
    }
    // option gemm_epi16: 16-bit results without a residual cross the epilogue's LDS transpose as 16-bit values (wave_epilogue16)
    if (!OUT_F32 && la::opts().gemm_epi16 && !((p.epilogue & LA_EPI_RESIDUAL) && p.residual)) p.epilogue |= LA_EPI_STAGE16;
    // cache-policy options of the 16-bit results (the encoder's QKV and MLP-up launches): a launch that sets one runs gemm_pp_kernel_cp
    if constexpr (!OUT_F32) {
        const int cp = ((p.epilogue & LA_EPI_STAGE16) ? (la::opts().cp_epi16 & PPCP_EPI16_MASK) : 0) | (duo && la::opts().cp_gemm_a ? PPCP_GEMM_A : 0);
        if (cp && (lnm == 0 || lnm == 2))
            return std::is_same<T16, bf16_t>::value ? launch_pp_cp_bf16(p, batch, lnm, duo, cp, stream) : launch_pp_cp_f16(p, batch, lnm, duo, cp, stream);
    }
    if (lnm == 2) return duo ? launch_pp_loop<OUT_F32, true, T16, 2>(p, batch, stream) : launch_pp_loop<OUT_F32, false, T16, 2>(p, batch, stream);
    if constexpr (OUT_F32) {
        if (lnm == 1) return duo ? launch_pp_loop<OUT_F32, true, T16, 1>(p, batch, stream) : launch_pp_loop<OUT_F32, false, T16, 1>(p, batch, stream);
    }
    return duo ? launch_pp_loop<OUT_F32, true, T16>(p, batch, stream) : launch_pp_loop<OUT_F32, false, T16>(p, batch, stream);
}

// la_gemm_split's launch: LNM = 3, (hi, lo) out
template <typename T16>
int launch_split(GemmParams p, int batch, hipStream_t stream) {
    const bool duo = p.K % 128 == 0 && p.K >= 256 && la::opts().gemm_loop != 99;
    if (const char *e = la::dev_env("LA_EPI_SPLIT_PASS")) { if (atoi(e) == 32) p.epilogue |= LA_EPI_SPLIT_PASS32; }
#ifdef LA_EXPERIMENTS
    if constexpr (std::is_same<T16, bf16_t>::value) {
        int rc = LA_OK;
        if (lab_try_launch(p, batch, true, 3, duo, stream, &rc)) return rc;
    }
#endif
    // cache-policy options of the split stream's producers (out-proj, MLP-down, the stem)
    const int cp = (la::opts().cp_split_st ? PPCP_SPLIT_ST : 0) | (la::opts().cp_split_ld && (p.epilogue & LA_EPI_SPLIT_INPLACE) ? PPCP_SPLIT_LD : 0) |
                   (duo && la::opts().cp_gemm_a ? PPCP_GEMM_A : 0);
    if (cp) return std::is_same<T16, bf16_t>::value ? launch_pp_cp_bf16(p, batch, 3, duo, cp, stream) : launch_pp_cp_f16(p, batch, 3, duo, cp, stream);
    return duo ? launch_pp_loop<true, true, T16, 3>(p, batch, stream) : launch_pp_loop<true, false, T16, 3>(p, batch, stream);
}

// The policy instantiations' dispatch (la_gemm_pp_cp_bf16.hip / la_gemm_pp_cp_f16.hip): cp's combinations per epilogue family.
template <bool OUT_F32, typename T16, int LNM, int CP>
int launch_pp_cp_one(const GemmParams &p, int batch, bool duo, hipStream_t stream) {
    if constexpr ((CP & PPCP_GEMM_A) != 0) return launch_pp_loop<OUT_F32, true, T16, LNM, CP>(p, batch, stream);      // (set for the hand-placed loop only)
    else return duo ? launch_pp_loop<OUT_F32, true, T16, LNM, CP>(p, batch, stream) : launch_pp_loop<OUT_F32, false, T16, LNM, CP>(p, batch, stream);
}
template <typename T16>
int launch_pp_cp(const GemmParams &p, int batch, int lnm, bool duo, int cp, hipStream_t stream) {
#define LA_PPCP_CASE(OUT_F32, LNM, CP) case CP: return launch_pp_cp_one<OUT_F32, T16, LNM, CP>(p, batch, duo, stream);
    if (lnm == 3) {
        switch (cp) {
            LA_PPCP_CASE(true, 3, 4) LA_PPCP_CASE(true, 3, 8) LA_PPCP_CASE(true, 3, 12) LA_PPCP_CASE(true, 3, 16)
            LA_PPCP_CASE(true, 3, 20) LA_PPCP_CASE(true, 3, 24) LA_PPCP_CASE(true, 3, 28)
        }
    } else if (lnm == 2) {
        switch (cp) { LA_PPCP_CASE(false, 2, 1) LA_PPCP_CASE(false, 2, 2) LA_PPCP_CASE(false, 2, 16) LA_PPCP_CASE(false, 2, 17) LA_PPCP_CASE(false, 2, 18) }
    } else if (lnm == 0) {
        switch (cp) { LA_PPCP_CASE(false, 0, 1) LA_PPCP_CASE(false, 0, 2) LA_PPCP_CASE(false, 0, 16) LA_PPCP_CASE(false, 0, 17) LA_PPCP_CASE(false, 0, 18) }
    }
#undef LA_PPCP_CASE
    la::set_error("gemm: no kernel for cache policy %d of epilogue family %d", cp, lnm);
    return LA_EINVAL;
}

}  // namespace gemm
}  // namespace la
