// la_attention.hip -- non-causal multi-head self-attention for the Whisper encoder
// (whisper.model.MultiHeadAttention.qkv_attention; head_dim = 64 for every model size),
// flash-style: the [T x T] score matrix never leaves the CU.
//
// Work split: grid = (ceil(T/128) query tiles, heads, clips); 4 waves per workgroup, each wave
// owns 32 query rows and sweeps the clip's keys in tiles of 64.  K and V tiles are staged by
// global_load_lds (16 B per lane) into a double-buffered, XOR-swizzled LDS image.
//
// The score tile is computed TRANSPOSED (S^T = K Q^T, 32 keys x 32 queries per MFMA) so that a
// lane holds one query's scores in its accumulator registers: the row max / row sum are
// register-local plus one cross-half exchange, and the exponentiated tile is directly the
// B-operand of O^T += V^T P^T (cdna guide, "An accumulator tile as the next MFMA's operand").
//   bf16: v_mfma_f32_32x32x16_bf16; V^T fragments come from ds_read_b64_tr_b16 on the row-major
//         V image; P is rounded to bf16 for the second product (f32 accumulate, f32 softmax).
//   f32 : v_mfma_f32_32x32x2_f32 (exact fmaf chains): parity mode, P stays f32.
// Softmax runs in the exp2 domain (v_exp_f32): p = exp2(s*log2e - m*log2e).
#include <type_traits>

#include "la_attn_tile.h"

using la::bf16_t;

namespace {

using namespace la::attn;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

// the two 16-bit operand types of the "throughput" kernels: same kernel text, different MFMA / conversion
template <typename T16> struct Half16;
template <> struct Half16<bf16_t> {
    typedef bf16x8 vec8;
    typedef __bf16 elem;
    static constexpr float kPLimit = 0x1p30f;        // optimistic softmax: largest row partial sum (hence P) taken without a redo
    __device__ static __forceinline__ f32x16 mfma32(vec8 a, vec8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Half16<la::f16_t> {
    typedef f16x8 vec8;
    typedef _Float16 elem;
    static constexpr float kPLimit = 0x1p13f;        // f16 tops out at 65504
    __device__ static __forceinline__ f32x16 mfma32(vec8 a, vec8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

#ifndef LA_ATTN_KO
#define LA_ATTN_KO 0      // timing-only builds (tools/ab_attn_knockouts.sh; results are garbage): bit mask of parts of the 16-bit tile loop
#endif                    // left out -- 1 exponentials, 2 V^T fragment reads, 4 K fragment reads, 8 staging after tile 0, 16 MFMAs, 32 barrier

struct AttnParams {
    const void *q, *k, *v;   // rows [clip*q_len + i][head*64 ..] / [clip*kv_len + j][head*64 ..]
    int64_t ld_q, ld_kv;
    void *out;
    int64_t ld_out;
    int q_len, kv_len, n_head, causal;
    int64_t q_bs, kv_bs, out_bs;   // rows from one clip to the next (== q_len / kv_len / q_len unless the caller says otherwise)
    int batch;
    float *lse = nullptr;       // float32 kernel, training forward: log sum_j exp(s_ij) per query row, [batch][n_head][q_len] (la_attention_bwd_f32)
    float score_scale = 1.4426950408889634f;   // 16-bit kernels: log2(e), or 1 when q already carries it (LA_Q_LOG2)
};

// NW = waves per workgroup (32 queries each): 4 (128 queries, 5 workgroups = 20 waves per CU by LDS) or 8 (256 queries: every
// K / V tile is staged once for twice the queries, 4 workgroups = 32 waves per CU)
// Optimistic softmax -- no per-tile maximum.  P = exp2(s log2 e - m_run) is formed against the running maximum as it
// stands and the row sums (needed anyway) are tested: only if some lane's partial sum is not <= LIMIT (a score rose far above
// the running maximum, or the first tile, where m_run = -inf gives +inf / NaN) is the tile redone the textbook way -- scores
// recomputed from the K tile still in LDS, maximum, rescale.  LIMIT keeps P inside the 16-bit type (2^30 for bf16, 2^13 for
// f16); the f32 accumulators and the final O / l are exact in the scale.
// FOLD (bf16, LA_Q_LOG2: q carries head_dim^-0.5 log2 e, so the scores arrive in the exp2 domain): the optimistic form with the
// running maximum STARTING AT 0 and, while no query of the wave has needed one, no subtraction at all -- P = exp2(s) as the scores
// come out of the matrix pipe.  bf16 has float32's exponent range, so P in 2^-126 .. 2^30 is as precise relative to its row as
// exp2(s - max) is; the float32 accumulators and the final O / l do not care about the common scale.  Per score that leaves
// v_exp_f32 + v_add_f32 (row sum) + half a v_cvt_pk on the vector pipe, the busier one here, instead of v_fma_f32 + those
// (337 -> 315 us per Whisper-medium layer).  Scores above 2^30 take the same redo path as before (it installs a maximum; from
// then on the wave subtracts it); a query whose scores ALL lie below ~2^-100 would underflow its sum: the block then repeats its
// sweep the textbook way (block-uniform decision after the sweep; never seen on real activations, forced in the tests).
// The forms measured slower than these (per-tile maximum with a deferred update, the denominator on the matrix pipe, raised wave
// priorities) are in profiles/NOTES.md and in the history of this file.
// CP: cache policy of the kernel's streamed accesses, compiled into the instruction text (la_common.h CachePol) -- bit 0 (option cp_attn_qo):
// the Q fragment loads and the output stores, each touched once per launch, are nt; bit 1 (option cp_attn_kv): the LDS-DMA pieces of the
// K / V tiles are nt.  The program is la_attention_body.h; attention_bf16_kernel is CP = 0, the instructions as they always were; attention_bf16_kernel_cp carries the others.
template <typename T16, int NW, bool FOLD>
__global__ __launch_bounds__(64 * NW, FOLD ? 4 : 2) void attention_bf16_kernel(AttnParams p) {
    constexpr int CP = 0;
#include "la_attention_body.h"
}
template <typename T16, int NW, bool FOLD, int CP>
__global__ __launch_bounds__(64 * NW, FOLD ? 4 : 2) void attention_bf16_kernel_cp(AttnParams p) {
    static_assert(CP != 0, "CP = 0 is attention_bf16_kernel");
#include "la_attention_body.h"
}

// ---------------------------------------------------------------------------------------------
// f32 (parity mode)
// ---------------------------------------------------------------------------------------------
// K / V images: [64 keys][256 B], 16-B slot s of row r stored at slot s ^ (r & 15).
__device__ __forceinline__ void stage_kv_f32(const float *kbase, const float *vbase, int64_t ld, int key0, int T,
                                             unsigned char *kl, unsigned char *vl, int wave, int lane) {
    const int r4 = lane >> 4, ps = lane & 15;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int piece = wave * 4 + i;
        const int r = piece * 4 + r4;
        int key = key0 + r;
        key = key < T ? key : T - 1;
        const int ls = ps ^ (r & 15);
        la::glds16(kbase + (int64_t)key * ld + (ls << 2), kl + piece * 1024);
        la::glds16(vbase + (int64_t)key * ld + (ls << 2), vl + piece * 1024);
    }
}

__global__ __launch_bounds__(256, 2) void attention_f32_kernel(AttnParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];  // [buf][K|V][64][256 B] = 64 KiB
    constexpr int QT = 128;   // queries per workgroup (4 waves x 32)
    const int T = p.kv_len;
    const BlockCoord bc = block_coord((p.q_len + QT - 1) / QT, p.n_head, p.batch);
    const int qt = bc.qt, head = bc.head, clip = bc.clip;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i32 = lane & 31, h = lane >> 5;
    const float *base = reinterpret_cast<const float *>(p.q) + (int64_t)clip * p.q_bs * p.ld_q + head * 64;
    const float *kbase = reinterpret_cast<const float *>(p.k) + (int64_t)clip * p.kv_bs * p.ld_kv + head * 64;
    const float *vbase = reinterpret_cast<const float *>(p.v) + (int64_t)clip * p.kv_bs * p.ld_kv + head * 64;

    int qrow = qt * QT + wave * 32 + i32;
    const bool q_valid = qrow < p.q_len;
    qrow = q_valid ? qrow : p.q_len - 1;
    // lane (q, h) holds Q[q][8c + 4h + e], c = 0..7, e = 0..3: element e feeds the e-th MFMA of chunk c
    float4 qf[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) qf[c] = *reinterpret_cast<const float4 *>(base + (int64_t)qrow * p.ld_q + 8 * c + 4 * h);

    f32x16 o[2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[b][r] = 0.f;
    float m_run = -INFINITY, l_part = 0.f;

    constexpr int TILE = KT * 256;
    int nkv = (T + KT - 1) / KT;
    if (p.causal) nkv = min(nkv, (min(p.q_len, (qt + 1) * QT) - 1) / KT + 1);
    stage_kv_f32(kbase, vbase, p.ld_kv, 0, T, lds, lds + TILE, wave, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    int cur = 0;
    for (int t = 0; t < nkv; ++t) {
        const unsigned char *kl = lds + cur * (2 * TILE);
        const unsigned char *vl = kl + TILE;
        if (t + 1 < nkv) {
            unsigned char *nk = lds + (cur ^ 1) * (2 * TILE);
            stage_kv_f32(kbase, vbase, p.ld_kv, (t + 1) * KT, T, nk, nk + TILE, wave, lane);
        }
        f32x16 s[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[sub][r] = 0.f;
            const int row = sub * 32 + i32;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float4 kf = *reinterpret_cast<const float4 *>(kl + row * 256 + (((2 * c + h) ^ (row & 15)) << 4));
                s[sub] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[c].x, s[sub], 0, 0, 0);
                s[sub] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[c].y, s[sub], 0, 0, 0);
                s[sub] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[c].z, s[sub], 0, 0, 0);
                s[sub] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[c].w, s[sub], 0, 0, 0);
            }
        }
        if ((t + 1) * KT > T || p.causal) {
            const int kmax = p.causal ? min(T - 1, qrow) : T - 1;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (t * KT + sub * 32 + acc_row(r, h) > kmax) s[sub][r] = -INFINITY;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[sub][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx * kLog2e);
        const float alpha = exp2f(m_run - m_new);
        m_run = m_new;
        float psum = 0.f;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = exp2f(fmaf(s[sub][r], kLog2e, -m_new));
                s[sub][r] = pv;
                psum += pv;
            }
        l_part = l_part * alpha + psum;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[b][r] *= alpha;
        // O^T += V^T P^T: MFMA `reg` contracts keys {acc_row(reg,0), acc_row(reg,1)}; B operand = s[sub][reg] as it stands,
        // A operand: lane (dv = 32b + i32, h) supplies V[key acc_row(reg,h)][dv]
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = sub * 32 + acc_row(r, h);
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int col = 32 * b + i32;  // dv
                    const float vv = *reinterpret_cast<const float *>(vl + key * 256 + ((((col >> 2) ^ (key & 15)) << 4) | ((col & 3) << 2)));
                    o[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv, s[sub][r], o[b], 0, 0, 0);
                }
            }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cur ^= 1;
    }

    const float l = l_part + __shfl_xor(l_part, 32);
    const float inv = 1.0f / l;
    if (p.lse && q_valid && h == 0)          // m_run is in the exp2 domain: lse = m ln 2 + ln l
        p.lse[((int64_t)clip * p.n_head + head) * p.q_len + qrow] = fmaf(m_run, 0.6931471805599453f, __logf(l));
    if (q_valid) {
        float *orow = reinterpret_cast<float *>(p.out) + ((int64_t)clip * p.out_bs + qrow) * p.ld_out + head * 64;
        store_row_scaled(orow, o, inv, h);
    }
}

}  // namespace

static int attention_launch(int dtype_arg, AttnParams p, int batch, hipStream_t stream) {
    const int dtype = dtype_arg & 0xff;
    const bool qlog2 = dtype_arg & LA_Q_LOG2;
    if (qlog2 && dtype != LA_BF16 && dtype != LA_F16) {
        la::set_error("attention: LA_Q_LOG2 goes with the 16-bit kernels");
        return LA_EINVAL;
    }
    p.score_scale = qlog2 ? 1.0f : kLog2e;
    p.batch = batch;
    if (dtype == LA_BF16 || dtype == LA_F16) {
        la::TimerScope ts("attention_bf16", stream);
        // 256-query workgroups of 8 waves where a sequence has at least four of them (the encoder: T = 1500): every K / V tile is
        // staged once for twice the queries -- two LDS-DMA pieces per wave and tile instead of four, and the GEMM knock-outs of
        // round 4 price a piece at 60-185 cycles of issue -- same results, 325 against 333 us per layer alone, -0.25 ms per step
        // same-box (profiles/r4_ab_attention_8_waves.txt).  Option attn_nw = 4 | 8 (LA_ATTN_NW) forces either form.
        const int nw_opt = la::opts().attn_nw;
        const int nw = nw_opt ? nw_opt : (p.q_len >= 1024 ? 8 : 4);
        const bool wide = nw == 8 && p.q_len >= 256;
        // [wide][bf16 | bf16 with exp2-domain scores (LA_Q_LOG2): no maximum until one is needed (FOLD) | f16]
        // [cache policy: bit 0 option cp_attn_qo, bit 1 option cp_attn_kv]
        typedef void (*Kernel)(AttnParams);
#define LA_ATTN_FORMS(CP)                                                                                                                                   \
    {{attention_bf16_kernel_cp<bf16_t, 4, false, CP>, attention_bf16_kernel_cp<bf16_t, 4, true, CP>, attention_bf16_kernel_cp<la::f16_t, 4, false, CP>}, \
     {attention_bf16_kernel_cp<bf16_t, 8, false, CP>, attention_bf16_kernel_cp<bf16_t, 8, true, CP>, attention_bf16_kernel_cp<la::f16_t, 8, false, CP>}}
        static const Kernel kForms[4][2][3] = {
            {{attention_bf16_kernel<bf16_t, 4, false>, attention_bf16_kernel<bf16_t, 4, true>, attention_bf16_kernel<la::f16_t, 4, false>},
             {attention_bf16_kernel<bf16_t, 8, false>, attention_bf16_kernel<bf16_t, 8, true>, attention_bf16_kernel<la::f16_t, 8, false>}},
            LA_ATTN_FORMS(1), LA_ATTN_FORMS(2), LA_ATTN_FORMS(3)};
#undef LA_ATTN_FORMS
        const int cp = (la::opts().cp_attn_qo ? 1 : 0) | (la::opts().cp_attn_kv ? 2 : 0);
        const int queries = wide ? 256 : 128;
        hipLaunchKernelGGL(kForms[cp][wide][dtype == LA_F16 ? 2 : qlog2], dim3(la::cdiv(p.q_len, queries) * p.n_head * batch), dim3(2 * queries), 0,
                           stream, p);
    } else {
        static la::DeviceOnce attr_once;
        if (attr_once.pending()) {
            LA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(attention_f32_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 4 * KT * 256));
            attr_once.mark();
        }
        la::TimerScope ts("attention_f32", stream);
        hipLaunchKernelGGL(attention_f32_kernel, dim3(la::cdiv(p.q_len, 128) * p.n_head * batch), dim3(256), 4 * KT * 256, stream, p);
    }
    LA_LAUNCH_CHECK();
    return LA_OK;
}

extern "C" int la_attention(int32_t dtype_arg, const void *qkv, int64_t ld_qkv, void *out, int64_t ld_out, int32_t batch,
                            int32_t frames, int32_t n_head, void *stream_) {
    if (batch == 0 || frames == 0) return LA_OK;
    if (const int rc = check_forward_args("attention", dtype_arg, qkv && out, qkv, qkv, qkv, out, ld_qkv, 3 * (int64_t)n_head * 64, ld_qkv, ld_out,
                                          batch, frames, frames, n_head, nullptr))
        return rc;
    const char *b = reinterpret_cast<const char *>(qkv);
    const int d = n_head * 64, es = (dtype_arg & 0xff) == LA_F32 ? 4 : 2;
    AttnParams p{b, b + (int64_t)d * es, b + (int64_t)2 * d * es, ld_qkv, ld_qkv, out, ld_out, frames, frames, n_head, 0, frames, frames, frames, 0};
    return attention_launch(dtype_arg, p, batch, (hipStream_t)stream_);
}

static const char kCausalSelf[] = "causal masking is defined for self-attention (q_len == kv_len)";

extern "C" int la_attention_ex(int32_t dtype_arg, const void *q, int64_t ld_q, const void *k, const void *v, int64_t ld_kv,
                               void *out, int64_t ld_out, int32_t batch, int32_t q_len, int32_t kv_len, int32_t n_head,
                               int32_t causal, void *stream_) {
    if (batch == 0 || q_len == 0) return LA_OK;
    if (const int rc = check_forward_args("attention_ex", dtype_arg, q && k && v && out, q, k, v, out, ld_q, n_head * 64, ld_kv, ld_out, batch, q_len,
                                          kv_len, n_head, causal && q_len != kv_len ? kCausalSelf : nullptr))
        return rc;
    AttnParams p{q, k, v, ld_q, ld_kv, out, ld_out, q_len, kv_len, n_head, causal ? 1 : 0, q_len, kv_len, q_len, 0};
    return attention_launch(dtype_arg, p, batch, (hipStream_t)stream_);
}

// The float32 forward of the TRAINING path: la_attention_ex that also hands over the row statistic the fused backward needs
// (lse [batch][n_head][q_len]), so that la_attention_bwd_f32 does not recompute the scores once more just for it.
extern "C" int la_attention_lse_f32(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, float *out, int64_t ld_out,
                                    int32_t batch, int32_t q_len, int32_t kv_len, int32_t n_head, int32_t causal, float *lse, void *stream_) {
    if (batch == 0 || q_len == 0) return LA_OK;
    if (const int rc = check_forward_args("attention_lse", LA_F32, q && k && v && out && lse, q, k, v, out, ld_q, n_head * 64, ld_kv, ld_out, batch,
                                          q_len, kv_len, n_head, causal && q_len != kv_len ? kCausalSelf : nullptr))
        return rc;
    AttnParams p{q, k, v, ld_q, ld_kv, out, ld_out, q_len, kv_len, n_head, causal ? 1 : 0, q_len, kv_len, q_len, 0};
    p.lse = lse;
    return attention_launch(LA_F32, p, batch, (hipStream_t)stream_);
}

// Attention against a key / value CACHE (autoregressive decoding, whisper/decoding.py's kv_cache): clip b's keys are rows
// [b * kv_batch_rows, b * kv_batch_rows + kv_len) of k / v -- the cache has room for kv_batch_rows >= kv_len rows per clip --
// and its queries rows [b * q_batch_rows, ... + q_len) of q; out rows are packed [b * q_len + i].  Queries are the LAST q_len
// positions of the sequence: with causal != 0 query i sees keys 0 .. kv_len - q_len + i.
extern "C" int la_attention_cached(int32_t dtype_arg, const void *q, int64_t ld_q, int64_t q_batch_rows, const void *k, const void *v,
                                   int64_t ld_kv, int64_t kv_batch_rows, void *out, int64_t ld_out, int32_t batch, int32_t q_len,
                                   int32_t kv_len, int32_t n_head, int32_t causal, void *stream_) {
    if (batch == 0 || q_len == 0) return LA_OK;
    const char *own = !(q_batch_rows >= q_len && kv_batch_rows >= kv_len) ? "batch strides shorter than the lengths"
                      : causal && q_len != 1 && q_len != kv_len           ? "causal masking needs q_len == 1 or q_len == kv_len"
                                                                          : nullptr;
    if (const int rc = check_forward_args("attention_cached", dtype_arg, q && k && v && out, q, k, v, out, ld_q, n_head * 64, ld_kv, ld_out, batch,
                                          q_len, kv_len, n_head, own))
        return rc;
    // one new token against the whole cache needs no mask at all
    AttnParams p{q, k, v, ld_q, ld_kv, out, ld_out, q_len, kv_len, n_head, (causal && q_len > 1) ? 1 : 0, q_batch_rows, kv_batch_rows, q_len, 0};
    return attention_launch(dtype_arg, p, batch, (hipStream_t)stream_);
}
