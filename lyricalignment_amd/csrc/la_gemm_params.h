// la_gemm_params.h -- launch parameters of the GEMM kernels and the entry points of the translation units they are built in:
// la_gemm.hip (host dispatch, the 128 x 128 kernel family incl. float32, split-K), la_gemm_pp_bf16.hip / la_gemm_pp_f16.hip (the
// 256 x 256 kernel per operand type: compiled in parallel), lab/la_gemm_lab.hip (experiment build only).
#pragma once
#include "la_common.h"

namespace la {
namespace gemm {

struct GemmParams {
    int M, N, K;
    const void *A;
    int64_t lda, strideA;
    const void *W;
    int64_t ldw, strideW;
    void *C;
    int64_t ldc, strideC;
    const float *bias;
    int64_t strideBias;
    const float *residual;
    int64_t ldr, strideR;
    int epilogue;
    int tiles_m, tiles_n, group;
    int mblock = 0;                    // ping-pong kernel: row tiles per M block of the tile order (tile_coord_mb; 0 = column groups over all of M)
    // LayerNorm folded into the GEMMs around it (ping-pong kernel only; la_gemm_fused_ln):
    void *C2 = nullptr;                // producer: second, 16-bit copy of the f32 result rows (the next GEMM's raw A operand)
    int64_t ldc2 = 0, strideC2 = 0;
    const float *ln_stats = nullptr;   // consumer: per-row (mean, rstd) of the raw A rows, [M][2]
    const float *ln_csum = nullptr;    // consumer: c[n] = sum_k W'[n][k] of the gamma-folded weights, [N]
    int K_tail = 0;                    // split-K: K of the LAST batch slot when the chunks are uneven (0 = p.K)
    int64_t plane_a = 0, plane_w = 0;  // f16x2 products (LNM 6): pitch in elements between the hi and the lo plane inside a row of A / W;
                                       // there ln_stats = per-row scales [M] and ln_csum = per-column scales [N] (powers of two)
    float *ln_part = nullptr;          // producer (optional): per-row partial statistics of the 16-bit copy, [N/64][M][2] =
                                       // (mean, sum of squared deviations) of each 64-column segment (la_ln_stats_finalize)
};

// Which kernel takes a product (DESIGN.md "Product routing"): the arithmetic every routing condition of the library is composed from.
// A site states its own conjunction of these (la_fc_emissions has no N term, la_gemm_split its own K term, ...); none restates a number.
constexpr int FILL_TILES = 192;        // 256 x 256 tiles (x batch slots) from which the 256 x 256 kernels fill the chip's 256 CUs
inline int64_t tiles256(int64_t M, int64_t N, int64_t slots = 1) { return (int64_t)la::cdiv(M, 256) * la::cdiv(N, 256) * slots; }
inline bool fills_chip(int64_t M, int64_t N, int64_t slots = 1) { return tiles256(M, N, slots) >= FILL_TILES; }
// K of the f16x2 products, per split-K slot: the 256 x 256 kernel walks whole 128-element chunks, at least two; the 128 x 128 one 32-element sub-stages
inline bool x2_k_ok(int K, int slots = 1) { return slots > 0 && K % slots == 0 && (K / slots) % 128 == 0 && K / slots >= 256; }
inline bool x2_small_k_ok(int K, int slots = 1) { return slots > 0 && K % slots == 0 && (K / slots) % 32 == 0; }
// la_gemm_f16x2's domain
inline bool x2_domain(int64_t M, int N, int K, int slots = 1) { return x2_k_ok(K, slots) && N > 128 && fills_chip(M, N, slots); }

// internal epilogue bits (beside the public LA_EPI_* of lyricalign.h)
constexpr int LA_EPI_SPLIT_INPLACE = 1 << 20;    // the residual is the split stream itself
constexpr int LA_EPI_SPLIT_PASS32 = 1 << 21;     // (experiment build, LA_EPI_SPLIT_PASS=32) the 32-row passes without the one-pass-ahead requests
constexpr int LA_EPI_STAGE16 = 1 << 22;         // option gemm_epi16: interior tiles of a 16-bit result without residual take wave_epilogue16
constexpr int LA_EPI_Q4_PRIO = 1 << 23;          // (experiment build, LA_GEMM_Q4_PRIO=1) gemm_q4_kernel's prologue / epilogue at wave priority 3
// Cache policy of a 256 x 256 launch (la_common.h CachePol; options cp_epi16, cp_split_st, cp_split_ld, cp_gemm_a), packed: the template
// argument of gemm_pp_kernel_cp, whose instantiations are built in la_gemm_pp_cp_bf16.hip / la_gemm_pp_cp_f16.hip.  0 = gemm_pp_kernel itself.
constexpr int PPCP_EPI16_MASK = 3;               // bits 0-1: stores of wave_epilogue16 (CP_NT | CP_WT)
constexpr int PPCP_SPLIT_ST = 4;                 // the split-stream epilogue's stores of the hi and lo planes: nt
constexpr int PPCP_SPLIT_LD = 8;                 // its loads of the incoming planes (in place): nt
constexpr int PPCP_GEMM_A = 16;                  // the hand-placed loop's LDS-DMA pieces of the A operand (waves 4-7): nt

// The 256 x 256 kernel by operand type (dtype: LA_BF16 | LA_F16).  launch_pp16: plain / LayerNorm-producer (p.C2) / LayerNorm-consumer
// (p.ln_stats) epilogues by p's fields; launch_split16: the split residual stream's producers (la_gemm_split; p.C = lo, p.C2 = hi).
int launch_pp_bf16(GemmParams p, int batch, bool out_f32, hipStream_t stream);
int launch_pp_f16(GemmParams p, int batch, bool out_f32, hipStream_t stream);
int launch_split_bf16(GemmParams p, int batch, hipStream_t stream);
int launch_split_f16(GemmParams p, int batch, hipStream_t stream);
// the same launches with a non-zero cache policy cp (PPCP_* above); lnm = 0 plain 16-bit result | 2 LayerNorm consumer | 3 split stream;
// p, duo as launch_pp / launch_split have prepared them
int launch_pp_cp_bf16(GemmParams p, int batch, int lnm, bool duo, int cp, hipStream_t stream);
int launch_pp_cp_f16(GemmParams p, int batch, int lnm, bool duo, int cp, hipStream_t stream);
// la_gemm_f16x2 (la_f32x2.hip): float32 products as three f16 products over segmented K, f32 out, scale epilogue; batch = split-K slots
int launch_x2_f16(GemmParams p, int batch, hipStream_t stream);

#ifdef LA_EXPERIMENTS
// lab/la_gemm_lab.hip: the measured-slower structures behind their per-launch developer switches (LA_GEMM_Q4, LA_GEMM_PERSIST,
// LA_PP_DBG=73, the in-loop LayerNorm statistics).  true = the launch was taken over (*rc = its status).
bool lab_try_launch(GemmParams &p, int batch, bool out_f32, int lnm, bool duo, hipStream_t stream, int *rc);
int lab_set_tile_stamps(void *buf);
#endif

}  // namespace gemm
}  // namespace la
