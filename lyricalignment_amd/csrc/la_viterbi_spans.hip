// la_viterbi_spans.hip -- the alignment DP of la_viterbi.hip on a lattice with OPTIONAL label spans (no counterpart in the
// reference, whose lattice makes every label occupy at least one frame).
//
// States as in la_viterbi.hip (0 = leading silence, 2n+1 = label n, 2n+2 = the silence after it).  skip_from[n] = a with
// 0 <= a < n declares labels a .. n-1 optional: the two states at position n (2n, and 2n+1 when n < L) get two more
// predecessors, J = 2a (the silence before the span) and J-1 = 2a-1 (the label before it; a >= 1, and for the odd target
// only when labels[n] != labels[a-1] -- the equal-neighbour rule).  Both are charged `penalty` and must beat the existing
// rule's winner strictly, J before J-1.  Float64 adds / subtracts in that order: results are reproducible to the bit.
//
// Mapping to the hardware: as viterbi_kernel -- one workgroup per clip, one lane per state, emissions prefetched PF frames
// ahead.  The single-wave form keeps the DPP shifts for k-1 / k-2 and fetches the jump sources with ds_bpermute of p0 and of
// the already-shifted p1 (lane J of p1 holds dp[J-1]).  "This clip has a span" is a workgroup-uniform test taken ONCE,
// outside the frame loop: a span-free clip runs a loop without any of the jump code.  The multi-wave forms read dp[J] /
// dp[J-1] from the LDS row they exchange anyway.  Backpointers are five outcomes {stay, advance, skip, jump from J, jump
// from J-1}: three 64-bit ballot masks per wave per frame (T * NW * 24 bytes; the third is written and read only where
// spans exist), in LDS when they fit, otherwise in the caller's workspace.  J(s) stays in an LDS int array for the
// backtrace thread.
#include <type_traits>

#include "la_common.h"

namespace {

constexpr double kNeg = -10000000.0;  // utils/alignment.py:144
constexpr int PF = 8;                 // emission prefetch depth (frames)

struct SpanParams {
    const float *em;
    int64_t em_bs, em_rs;
    const int32_t *labels;
    int32_t labels_stride;
    const int32_t *n_labels;
    const int32_t *n_frames;
    int32_t max_frames, max_labels;
    int32_t *onset, *offset;
    int32_t out_stride;
    double *final_score;
    int32_t *status;
    const int32_t *skip_from;
    int32_t skip_stride;
    double penalty;
    unsigned long long *bt_global;  // [batch][max_frames][NW][3] when !bt_in_lds
    int32_t bt_in_lds;
};

__device__ __forceinline__ double wave_shr1(double x) {
    int lo = __double2loint(x), hi = __double2hiint(x);
    // DPP wave_shr:1 -- lane i receives lane i-1 across the whole wave64 (gfx9 family)
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// lane i receives x of lane (byte_addr / 4); byte_addr is always a lane of this wave
__device__ __forceinline__ double wave_gather(double x, int byte_addr) {
    const int lo = __builtin_amdgcn_ds_bpermute(byte_addr, __double2loint(x));
    const int hi = __builtin_amdgcn_ds_bpermute(byte_addr, __double2hiint(x));
    return __hiloint2double(hi, lo);
}

constexpr int kSkipped = -2;  // off_s marker of a label inside a taken jump (written out as -1)

template <int NW, bool DPP>
__global__ __launch_bounds__(NW * 64) void viterbi_spans_kernel(SpanParams p) {
    static_assert(!DPP || NW == 1, "DPP neighbour exchange is single-wave only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NT = NW * 64;
    // carve: row exchange [2][NT+2] f64 | on/off [2][max_labels] i32 | J [NT] i32 | bt masks
    double *rowbuf = reinterpret_cast<double *>(smem);
    int32_t *on_s = reinterpret_cast<int32_t *>(smem + 2 * (NT + 2) * sizeof(double));
    const int Lpad = (p.max_labels + 3) & ~3;
    int32_t *off_s = on_s + Lpad;
    int32_t *j_s = off_s + Lpad;
    unsigned long long *bt_lds = reinterpret_cast<unsigned long long *>(j_s + NT);

    const int b = blockIdx.x;
    const int k = threadIdx.x;
    const int wave = k >> 6;
    const int lane = k & 63;
    const int L = p.n_labels[b];
    const int T = p.n_frames[b];
    const int S = 2 * L + 1;

    for (int n = k; n < p.max_labels; n += NT) {
        p.onset[(int64_t)b * p.out_stride + n] = -1;
        p.offset[(int64_t)b * p.out_stride + n] = -1;
        on_s[n] = -1;
        off_s[n] = -1;
    }
    if (L <= 0) {
        if (k == 0) { p.status[b] = LA_EEMPTY; p.final_score[b] = 0.0; }
        return;
    }
    if (T <= 0 || T > p.max_frames || L > p.max_labels || S > NT) {
        if (k == 0) { p.status[b] = LA_EINVAL; p.final_score[b] = 0.0; }
        return;
    }

    unsigned long long *bt = p.bt_in_lds ? bt_lds : p.bt_global + (int64_t)b * p.max_frames * NW * 3;

    const bool valid = k < S;
    const bool odd = (k & 1) != 0;
    const int n = k >> 1;
    const int col = (odd && valid) ? 1 + n : 0;
    const int32_t *lab = p.labels + (int64_t)b * p.labels_stride;
    bool can_skip = false;  // label[k//2] != label[k//2-1], odd k >= 3
    if (odd && valid && k >= 3) can_skip = lab[n] != lab[n - 1];
    // the span that ends at this state's position n (n <= L for every valid state); anything outside 0 <= a < n is "none"
    int J = -1;
    bool jm1_ok = false;
    if (valid && n >= 1) {
        const int a = p.skip_from[(int64_t)b * p.skip_stride + n];
        if (a >= 0 && a < n) {
            J = 2 * a;
            jm1_ok = a >= 1 && (!odd || lab[n] != lab[a - 1]);
        }
    }
    j_s[k] = J;
    const double pen = p.penalty;
    const float *emb = p.em + (int64_t)b * p.em_bs + col;

    double cur = (k <= 1) ? (double)emb[0] : kNeg;

    if (!DPP) {
        if (k < 2) { rowbuf[k] = kNeg; rowbuf[NT + 2 + k] = kNeg; }  // slots for k-1, k-2 of states 0,1
    }
    // workgroup-uniform (one wave: a ballot): a clip without a span runs a frame loop without any of the jump code
    const bool has_span = NW == 1 ? __ballot(J >= 0) != 0ull : __syncthreads_or(J >= 0) != 0;
    const int gather_addr = (J >= 0 ? J : lane) << 2;   // (single wave: J < S <= 64)

    float e_buf[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        const int jj = 1 + i;
        e_buf[i] = jj < T ? emb[(int64_t)jj * p.em_rs] : 0.0f;
    }
    int parity = 0;
    auto sweep = [&](auto has_c) {
        constexpr bool HAS = decltype(has_c)::value;
        for (int j0 = 1; j0 < T; j0 += PF) {
            float e_cur[PF];
#pragma unroll
            for (int i = 0; i < PF; ++i) e_cur[i] = e_buf[i];
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const int jj = j0 + PF + i;
                e_buf[i] = jj < T ? emb[(int64_t)jj * p.em_rs] : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const int j = j0 + i;
                if (j >= T) break;
                double p0 = cur, p1, p2, pj = kNeg, pjm1 = kNeg;
                if (DPP) {
                    p1 = wave_shr1(p0);
                    p2 = wave_shr1(p1);
                    if (HAS) {
                        pj = wave_gather(p0, gather_addr);
                        pjm1 = wave_gather(p1, gather_addr);   // lane J of the shifted row holds dp[J-1]
                    }
                } else {
                    double *rb = rowbuf + parity * (NT + 2);
                    rb[k + 2] = p0;
                    __syncthreads();
                    p1 = rb[k + 1];
                    p2 = rb[k];
                    if (HAS && J >= 0) {
                        pj = rb[J + 2];
                        pjm1 = rb[J + 1];
                    }
                    parity ^= 1;
                }
                const bool stay = p0 > p1;                                   // strict
                const bool skip = can_skip && (p2 >= p1) && (p2 >= p0);
                int code = skip ? 2 : (stay ? 0 : 1);
                double best = skip ? p2 : (stay ? p0 : p1);
                if (k == 0) { code = 0; best = p0; }
                if (HAS && J >= 0) {
                    const double vj = pj - pen;
                    if (vj > best) { best = vj; code = 3; }                  // strict, J before J-1
                    if (jm1_ok) {
                        const double vm = pjm1 - pen;
                        if (vm > best) { best = vm; code = 4; }
                    }
                }
                cur = best + (double)e_cur[i];
                const unsigned long long m0 = __ballot(code & 1);
                const unsigned long long m1 = __ballot((code >> 1) & 1);
                unsigned long long m2 = 0ull;
                if (HAS) m2 = __ballot(code >> 2);
                if (lane == 0) {
                    unsigned long long *row = bt + ((int64_t)j * NW + wave) * 3;
                    row[0] = m0;
                    row[1] = m1;
                    if (HAS) row[2] = m2;                                    // (read back only for states with a span)
                }
            }
        }
    };
    if (has_span) sweep(std::true_type{});
    else sweep(std::false_type{});

    // termination + backtrace by one thread
    __syncthreads();
    double *fin = rowbuf;
    fin[k] = cur;
    __threadfence_block();
    __syncthreads();
    if (k == 0) {
        int kk = (fin[S - 1] > fin[S - 2]) ? (S - 1) : (S - 2);  // strict '>'
        p.final_score[b] = fin[kk];
        int knext = -1;
        for (int j = T - 1; j >= 0; --j) {
            if (kk & 1) {
                const int nn = kk >> 1;
                if (kk != knext) off_s[nn] = j + 1;  // last frame in this state + 1
                on_s[nn] = j;                        // keeps decreasing to the first frame
            }
            knext = kk;
            if (j > 0) {
                const unsigned long long *row = bt + ((int64_t)j * NW + (kk >> 6)) * 3;
                const int sh = kk & 63;
                int code = (int)((row[0] >> sh) & 1ull) | ((int)((row[1] >> sh) & 1ull) << 1);
                if (has_span) {                      // (uniform: a span-free clip's backtrace is la_viterbi.hip's)
                    const int Jk = j_s[kk];          // the third mask exists only where spans do
                    if (Jk >= 0) code |= (int)((row[2] >> sh) & 1ull) << 2;
                    if (code >= 3) {
                        for (int m = Jk >> 1; m < (kk >> 1); ++m) off_s[m] = kSkipped;
                        code = kk - (Jk - (code - 3));
                    }
                }
                kk -= code;
            }
        }
        int st = LA_OK;
        for (int nn = 0; nn < L; ++nn) {
            if (off_s[nn] == kSkipped) off_s[nn] = -1;
            else if (on_s[nn] < 0) st = LA_EINFEASIBLE;
        }
        p.status[b] = st;
    }
    __syncthreads();
    for (int nn = k; nn < L; nn += NT) {
        p.onset[(int64_t)b * p.out_stride + nn] = on_s[nn];
        p.offset[(int64_t)b * p.out_stride + nn] = off_s[nn];
    }
}

struct SpanPlan {
    int nw;
    bool bt_in_lds;
    size_t lds_bytes;
    size_t ws_bytes;
};

constexpr size_t kLdsBudget = 160 * 1024 - 1024;   // la_viterbi.hip's
constexpr int kMaxLabels = 511;                    // one lane per lattice state, 1024 states per workgroup

bool plan_spans(int batch, int max_frames, int max_labels, SpanPlan *pl) {
    if (max_labels > kMaxLabels) return false;
    const int S = 2 * max_labels + 1;
    int nw = 1;
    while (nw * 64 < S) nw *= 2;
    const size_t fixed = 2 * (size_t)(nw * 64 + 2) * sizeof(double) + 2 * (size_t)((max_labels + 3) & ~3) * sizeof(int32_t) +
                         (size_t)nw * 64 * sizeof(int32_t);
    const size_t fixed_al = (fixed + 15) & ~(size_t)15;
    const size_t bt_bytes = (size_t)max_frames * nw * 24;
    pl->nw = nw;
    pl->bt_in_lds = fixed_al + bt_bytes <= kLdsBudget;
    pl->lds_bytes = pl->bt_in_lds ? fixed_al + bt_bytes : fixed_al;
    pl->ws_bytes = pl->bt_in_lds ? 0 : (size_t)batch * bt_bytes;
    return true;
}

template <int NW, bool DPP>
int launch_spans(const SpanParams &p, const SpanPlan &pl, int batch, hipStream_t stream) {
    auto kern = viterbi_spans_kernel<NW, DPP>;
    static la::DeviceOnce attr_once;            // once per instantiation, to the planner's budget (pl.lds_bytes never exceeds it)
    if (pl.lds_bytes > 48 * 1024 && attr_once.pending()) {
        LA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
        attr_once.mark();
    }
    la::TimerScope ts("viterbi_spans", stream);
    hipLaunchKernelGGL(kern, dim3(batch), dim3(NW * 64), pl.lds_bytes, stream, p);
    LA_LAUNCH_CHECK();
    return LA_OK;
}

}  // namespace

extern "C" int la_viterbi_spans_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    LA_CHECK_ARG(bytes && batch >= 0 && max_frames > 0 && max_labels > 0, "viterbi_spans_workspace_bytes: bad arguments");
    SpanPlan pl;
    if (!plan_spans(batch, max_frames, max_labels, &pl)) {
        la::set_error("viterbi_spans: max_labels %d exceeds %d (one lane per lattice state)", max_labels, kMaxLabels);
        return LA_EUNSUPPORTED;
    }
    *bytes = pl.ws_bytes;
    return LA_OK;
}

extern "C" int la_viterbi_spans_batch(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                                      const int32_t *labels, int32_t labels_stride, const int32_t *n_labels,
                                      const int32_t *n_frames, int32_t batch, int32_t max_frames, int32_t max_labels,
                                      int32_t *onset, int32_t *offset, int32_t out_stride, double *final_score,
                                      int32_t *status, const int32_t *skip_from, int32_t skip_stride, double skip_penalty,
                                      void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (batch == 0) return LA_OK;
    LA_CHECK_ARG(em && labels && n_labels && n_frames && onset && offset && final_score && status && skip_from,
                 "viterbi_spans_batch: null pointer");
    LA_CHECK_ARG(batch > 0 && max_frames > 0 && max_labels > 0, "viterbi_spans_batch: bad sizes");
    LA_CHECK_ARG(skip_penalty >= 0.0, "viterbi_spans_batch: skip_penalty must be >= 0 (and not NaN)");
    SpanPlan pl;
    if (!plan_spans(batch, max_frames, max_labels, &pl)) {
        la::set_error("viterbi_spans: max_labels %d exceeds %d (one lane per lattice state)", max_labels, kMaxLabels);
        return LA_EUNSUPPORTED;
    }
    LA_CHECK_ARG(em_row_stride >= max_labels + 1 && out_stride >= max_labels && labels_stride >= max_labels &&
                     skip_stride >= max_labels + 1,
                 "viterbi_spans_batch: strides smaller than max_labels");
    LA_CHECK_ARG(pl.ws_bytes == 0 || (workspace && workspace_bytes >= pl.ws_bytes),
                 "viterbi_spans_batch: workspace too small (%zu < %zu)", workspace_bytes, pl.ws_bytes);
    LA_CHECK_ARG(pl.ws_bytes == 0 || (uintptr_t)workspace % 8 == 0, "viterbi_spans_batch: workspace must be 8-byte aligned");
    SpanParams p{em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames,
                 max_labels, onset, offset, out_stride, final_score, status, skip_from, skip_stride, skip_penalty,
                 reinterpret_cast<unsigned long long *>(workspace), pl.bt_in_lds ? 1 : 0};
    const bool no_dpp = !la::opts().viterbi_dpp;
    switch (pl.nw) {
        case 1: return no_dpp ? launch_spans<1, false>(p, pl, batch, stream) : launch_spans<1, true>(p, pl, batch, stream);
        case 2: return launch_spans<2, false>(p, pl, batch, stream);
        case 4: return launch_spans<4, false>(p, pl, batch, stream);
        case 8: return launch_spans<8, false>(p, pl, batch, stream);
        case 16: return launch_spans<16, false>(p, pl, batch, stream);
    }
    return LA_EUNSUPPORTED;
}
