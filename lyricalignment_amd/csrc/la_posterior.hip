// la_posterior.hip -- per-character alignment confidence for gfx950: forward-backward (sum-product) on the DP's lattice.
//
// la_viterbi.hip sweeps the lattice of utils/alignment.py:73-119,144-157 max-product and reports ONE path.  The same lattice
// swept sum-product gives the posterior probability gamma_t(k) of every (frame, state) cell under the model, and from it a
// normalised number per character: how much of the model's belief lies inside the reported segment (occupancy) and how much
// of the first-frame / last-frame distribution of the label lies within `boundary_window` frames of the reported onset /
// offset (onset_prob / offset_prob).  The reference has no counterpart (its alignment is max-product only).
//
// Mapping to the hardware (DESIGN.md "Alignment posteriors"): one workgroup per utterance, one lane per lattice state, two
// dependent sweeps of T steps.  Forward: alpha rows to the caller's float64 workspace [batch][max_frames][S_pad].  Backward:
// beta stays in a register; per step every lane forms its gamma, every label lane also its exit term (from the two shifted
// beta_{t+1} values the recurrence fetched anyway) and its entry term (from the stored alpha_{t-1} row one and two states
// down) and adds them to three lane-local sums while t lies inside the label's segment / windows.  No atomics, no second
// pass, one store per label at the end.  S <= 64: ONE wave64, neighbours by DPP wave shifts, no LDS and no barrier in the
// loops.  64 < S <= 1024: up to 16 waves, the previous row through a double-buffered float64 row in LDS, one barrier per
// frame.  Emissions and stored alpha rows are prefetched a block of steps (8; 4 in the multi-wave form) ahead of the dependency chain.
//
// Arithmetic: path scores are float64 (they reach -T * 35).  The log-sum-exp of a step takes its maximum in float64 and the
// correction log(sum exp(x - max)), which lies in [0, ln 3], in float32 (la_lattice.h log_add3, shared with la_loss.hip): <= ~1e-7 absolute per step,
// and a third of the float64 exp / log latency on a kernel that is nothing but a 2T-step latency chain.  Unreachable cells
// are -inf (weight zero); the DP's finite -1e7 is a max-product device and does not appear here.
#include "la_lattice.h"

namespace {

using namespace la::lattice;

struct PostParams {
    const float *em;
    int64_t em_bs, em_rs;
    const int32_t *labels;
    int32_t labels_stride;
    const int32_t *n_labels;
    const int32_t *n_frames;
    int32_t max_frames, max_labels;
    const int32_t *onset, *offset;
    int32_t out_stride;
    int32_t window;
    float *occupancy, *onset_prob, *offset_prob;
    double *log_z;
    int32_t *status;
    float *gamma;
    int64_t gamma_bs, gamma_rs;
    double *alpha_ws;  // [batch][max_frames][NT]
};

template <int NW, bool DPP>
__global__ __launch_bounds__(NW * 64) void posterior_kernel(PostParams p) {
    static_assert(!DPP || NW == 1, "DPP neighbour exchange is single-wave only");
    constexpr int NT = NW * 64;
    constexpr int U = DPP ? 8 : 4;  // steps per prefetch block (the multi-wave form also prefetches two neighbour alpha columns: 1024 threads leave 128 VGPRs)
    // own state at [k + 2]; [0], [1] and [NT + 2], [NT + 3] stay -inf: the neighbours of the first / last states
    __shared__ double rowbuf[DPP ? 1 : 2][DPP ? 1 : NT + 4];
    __shared__ double fin[2];

    const int b = blockIdx.x;
    const int k = threadIdx.x;
    const int L = p.n_labels[b];
    const int T = p.n_frames[b];
    const int S = 2 * L + 1;
    const int Sg = 2 * p.max_labels + 1;  // <= NT (planned from max_labels)
    const bool odd = (k & 1) != 0;
    const int n = k >> 1;
    const double NEG = -INFINITY;

    float *occ_g = p.occupancy + (int64_t)b * p.out_stride;
    float *onp_g = p.onset_prob + (int64_t)b * p.out_stride;
    float *offp_g = p.offset_prob + (int64_t)b * p.out_stride;
    float *gam = p.gamma ? p.gamma + (int64_t)b * p.gamma_bs : nullptr;
    const bool row_lane = odd && n < p.max_labels;  // the lane that writes label row n (every n < max_labels has one)
    auto zero_gamma_from = [&](int t_from) {
        if (gam && k < Sg)
            for (int t = t_from; t < p.max_frames; ++t) gam[(int64_t)t * p.gamma_rs + k] = 0.f;
    };
    auto fail = [&](int st, double lz) {
        if (row_lane) { occ_g[n] = 0.f; onp_g[n] = 0.f; offp_g[n] = 0.f; }
        zero_gamma_from(0);
        if (k == 0) { p.status[b] = st; p.log_z[b] = lz; }
    };
    if (L <= 0) { fail(LA_EEMPTY, 0.0); return; }
    if (T <= 0 || T > p.max_frames || L > p.max_labels) { fail(LA_EINVAL, 0.0); return; }

    const bool valid = k < S;
    const int col = (odd && valid) ? 1 + n : 0;
    const int32_t *lab = p.labels + (int64_t)b * p.labels_stride;
    const bool can_skip = odd && valid && k >= 3 && lab[n] != lab[n - 1];           // k-2 -> k
    const bool can_skip_from = odd && valid && (k + 2 < S) && lab[n + 1] != lab[n];  // k -> k+2
    const float *emb = p.em + (int64_t)b * p.em_bs + col;
    double *aw = p.alpha_ws + (int64_t)b * p.max_frames * NT + k;   // every lane owns a column (k >= S: -inf)

    int parity = 0;
    if (!DPP) {
        if (k < 2) {
            rowbuf[0][k] = NEG; rowbuf[1][k] = NEG;
            rowbuf[0][NT + 2 + k] = NEG; rowbuf[1][NT + 2 + k] = NEG;
        }
    }

    // ---- forward: alpha_t(k) = e_t(k) + logsumexp(alpha_{t-1}(k), alpha_{t-1}(k-1), [alpha_{t-1}(k-2)]) ----
    double a = k <= 1 ? (double)emb[0] : NEG;
    aw[0] = a;
    {
        float ev[U];
        auto fetch = [&](int t0) {
#pragma unroll
            for (int u = 0; u < U; ++u) ev[u] = emb[(int64_t)min(t0 + u, T - 1) * p.em_rs];
        };
        fetch(1);
        for (int t0 = 1; t0 < T; t0 += U) {
            float ec[U];
#pragma unroll
            for (int u = 0; u < U; ++u) ec[u] = ev[u];
            if (t0 + U < T) fetch(t0 + U);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u;
                if (t < T) {  // workgroup-uniform
                    double a1, a2;
                    if (DPP) {
                        a1 = wave_shr1(a, NEG);
                        a2 = wave_shr1(a1, NEG);
                    } else {
                        double *rb = rowbuf[DPP ? 0 : parity];
                        rb[k + 2] = a;
                        __syncthreads();
                        a1 = rb[k + 1];
                        a2 = rb[k];
                        parity ^= 1;
                    }
                    if (!can_skip) a2 = NEG;
                    a = valid ? log_add3(a, a1, a2) + (double)ec[u] : NEG;
                    aw[(int64_t)t * NT] = a;
                }
            }
        }
    }
    if (k == S - 1) fin[0] = a;
    if (k == S - 2) fin[1] = a;
    __threadfence_block();   // the backward sweep of the multi-wave form reads alpha columns written by other lanes
    __syncthreads();
    const double log_z = log_add(fin[0], fin[1]);
    if (log_z == -INFINITY) { fail(LA_EINFEASIBLE, log_z); return; }  // no path at all: T too short for the labels

    // ---- backward: beta in a register, gamma / entry / exit per step, lane-local sums ----
    int on = -1, off = -1;
    if (odd && valid) { on = p.onset[(int64_t)b * p.out_stride + n]; off = p.offset[(int64_t)b * p.out_stride + n]; }
    const bool acc_lane = odd && valid && on >= 0 && off > on;
    const int off_last = off - 1, w = p.window;
    double s_occ = 0.0, s_on = 0.0, s_off = 0.0;
    double be = NEG;
    {
        float ev[U];
        double av[U + 1];                 // alpha_t(k) for t = t0 .. t0 - U (the last one is alpha_{t-1} of the block's last step)
        double av1[DPP ? 1 : U], av2[DPP ? 1 : U];  // multi-wave form: alpha_{t-1}(k-1), alpha_{t-1}(k-2) straight from the workspace
        auto fetch = [&](int t0) {  // steps t0, t0 - 1, ..., t0 - U + 1
#pragma unroll
            for (int u = 0; u < U; ++u) ev[u] = emb[(int64_t)max(t0 - u, 0) * p.em_rs];
#pragma unroll
            for (int u = 0; u <= U; ++u) av[u] = aw[(int64_t)max(t0 - u, 0) * NT];
            if (!DPP) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t r = (int64_t)max(t0 - u - 1, 0) * NT;
                    av1[u] = k >= 1 ? aw[r - 1] : NEG;
                    av2[u] = k >= 2 ? aw[r - 2] : NEG;
                }
            }
        };
        fetch(T - 1);
        for (int t0 = T - 1; t0 >= 0; t0 -= U) {
            float ec[U];
            double ac[U + 1], ac1[DPP ? 1 : U], ac2[DPP ? 1 : U];
#pragma unroll
            for (int u = 0; u < U; ++u) ec[u] = ev[u];
#pragma unroll
            for (int u = 0; u <= U; ++u) ac[u] = av[u];
            if (!DPP) {
#pragma unroll
                for (int u = 0; u < U; ++u) { ac1[u] = av1[u]; ac2[u] = av2[u]; }
            }
            if (t0 - U >= 0) fetch(t0 - U);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 - u;
                if (t >= 0) {  // workgroup-uniform
                    const double e = (double)ec[u];
                    const double at = ac[u];
                    double out = NEG;  // log weight of leaving state k after frame t: beta_{t+1}(k+1), [beta_{t+1}(k+2)]
                    if (t == T - 1) {
                        be = (k == S - 1 || k == S - 2) ? e : NEG;
                    } else {
                        double b1, b2;
                        if (DPP) {
                            b1 = wave_shl1(be, NEG);
                            b2 = wave_shl1(b1, NEG);
                        } else {
                            double *rb = rowbuf[DPP ? 0 : parity];
                            rb[k + 2] = be;
                            __syncthreads();
                            b1 = rb[k + 3];
                            b2 = rb[k + 4];
                            parity ^= 1;
                        }
                        if (!can_skip_from) b2 = NEG;
                        out = log_add2(b1, b2);
                        be = valid ? log_add3(be, b1, b2) + e : NEG;
                    }
                    double am1, am2;  // alpha_{t-1}(k-1), alpha_{t-1}(k-2)
                    if (DPP) {
                        am1 = wave_shr1(ac[u + 1], NEG);
                        am2 = wave_shr1(am1, NEG);
                    } else {
                        am1 = ac1[u];
                        am2 = ac2[u];
                    }
                    const float g = __expf((float)(at + be - e - log_z));  // alpha and beta both include e_t(k)
                    if (gam && k < Sg) gam[(int64_t)t * p.gamma_rs + k] = g;
                    if (acc_lane) {
                        if (t >= on && t < off) s_occ += (double)g;
                        if (abs(t - on) <= w) {
                            float en = g;
                            if (t > 0) en = __expf((float)(log_add2(am1, can_skip ? am2 : NEG) + be - log_z));
                            s_on += (double)en;
                        }
                        if (abs(t - off_last) <= w) {
                            const float ex = t == T - 1 ? g : __expf((float)(at + out - log_z));
                            s_off += (double)ex;
                        }
                    }
                }
            }
        }
    }
    if (row_lane) {
        occ_g[n] = acc_lane ? (float)(s_occ / (double)(off - on)) : 0.f;
        onp_g[n] = acc_lane ? (float)s_on : 0.f;
        offp_g[n] = acc_lane ? (float)s_off : 0.f;
    }
    zero_gamma_from(T);
    if (k == 0) { p.status[b] = LA_OK; p.log_z[b] = log_z; }
}

// one lane per state; false above 16 waves
bool plan_posterior(int max_labels, int *nw_out) {
    *nw_out = waves_for_labels(max_labels);
    return *nw_out <= 16;
}

template <int NW, bool DPP>
int launch_posterior(const PostParams &p, int batch, hipStream_t stream) {
    la::TimerScope ts("posterior", stream);
    hipLaunchKernelGGL((posterior_kernel<NW, DPP>), dim3(batch), dim3(NW * 64), 0, stream, p);
    LA_LAUNCH_CHECK();
    return LA_OK;
}

}  // namespace

extern "C" int la_alignment_posteriors_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    LA_CHECK_ARG(bytes && batch >= 0 && max_frames > 0 && max_labels > 0, "alignment_posteriors_workspace_bytes: bad arguments");
    int nw;
    if (!plan_posterior(max_labels, &nw)) {
        la::set_error("alignment_posteriors: max_labels %d exceeds 511 (one lane per lattice state, 1024 states per workgroup)", max_labels);
        return LA_EUNSUPPORTED;
    }
    *bytes = (size_t)batch * (size_t)max_frames * (size_t)(nw * 64) * sizeof(double);
    return LA_OK;
}

extern "C" int la_alignment_posteriors(const float *em, int64_t em_batch_stride, int64_t em_row_stride, const int32_t *labels,
                                       int32_t labels_stride, const int32_t *n_labels, const int32_t *n_frames, int32_t batch,
                                       int32_t max_frames, int32_t max_labels, const int32_t *onset, const int32_t *offset,
                                       int32_t out_stride, int32_t boundary_window, float *occupancy, float *onset_prob,
                                       float *offset_prob, double *log_z, int32_t *status, float *gamma_out,
                                       int64_t gamma_batch_stride, int64_t gamma_row_stride, void *workspace,
                                       size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (batch == 0) return LA_OK;
    LA_CHECK_ARG(em && labels && n_labels && n_frames && onset && offset, "alignment_posteriors: null input pointer");
    LA_CHECK_ARG(occupancy && onset_prob && offset_prob && log_z && status, "alignment_posteriors: null output pointer");
    LA_CHECK_ARG(batch > 0 && max_frames > 0 && max_labels > 0, "alignment_posteriors: bad sizes");
    LA_CHECK_ARG(boundary_window >= 0, "alignment_posteriors: negative boundary_window");
    LA_CHECK_ARG(em_row_stride >= max_labels + 1 && out_stride >= max_labels && labels_stride >= max_labels,
                 "alignment_posteriors: strides smaller than max_labels");
    LA_CHECK_ARG(!gamma_out || (gamma_row_stride >= 2 * (int64_t)max_labels + 1 &&
                                (batch == 1 || gamma_batch_stride >= (int64_t)max_frames * gamma_row_stride)),
                 "alignment_posteriors: gamma strides smaller than [max_frames][2 max_labels + 1]");
    int nw;
    if (!plan_posterior(max_labels, &nw)) {
        la::set_error("alignment_posteriors: max_labels %d exceeds 511", max_labels);
        return LA_EUNSUPPORTED;
    }
    const size_t need = (size_t)batch * (size_t)max_frames * (size_t)(nw * 64) * sizeof(double);
    LA_CHECK_ARG(workspace && workspace_bytes >= need, "alignment_posteriors: workspace too small (%zu < %zu)", workspace_bytes, need);
    LA_CHECK_ARG((uintptr_t)workspace % 8 == 0, "alignment_posteriors: workspace must be 8-byte aligned");
    PostParams p{em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels,
                 onset, offset, out_stride, boundary_window, occupancy, onset_prob, offset_prob, log_z, status,
                 gamma_out, gamma_batch_stride, gamma_row_stride, reinterpret_cast<double *>(workspace)};
    switch (nw) {
        case 1: return la::opts().viterbi_dpp ? launch_posterior<1, true>(p, batch, stream) : launch_posterior<1, false>(p, batch, stream);
        case 2: return launch_posterior<2, false>(p, batch, stream);
        case 4: return launch_posterior<4, false>(p, batch, stream);
        case 8: return launch_posterior<8, false>(p, batch, stream);
        case 16: return launch_posterior<16, false>(p, batch, stream);
    }
    return LA_EUNSUPPORTED;
}
