// la_anchor_loss.hip -- training from line times: the negative log-partition of the lattice with per-state frame windows as a loss on the
// framewise align logits, forward AND gradient w.r.t. the logits (la_anchored_alignment_loss; DESIGN.md "Alignment loss on the windowed
// lattice").  The reference has no counterpart: its fine-tune losses need a label for every frame (la_loss.hip).
//
//   em       the CTC-variant compact emissions of la_emissions_from_logits, bit for bit (V word columns incl. column 0, silence logit at V):
//              em[t][0]   = logsigmoid(x[t][V])
//              em[t][1+n] = x[t][c_n] - lse_{1..V-1}(x[t]) + logsigmoid(-x[t][V])
//   nll_b    = -log_z_b, the windowed log-partition of la_alignment_posteriors_windows on em
//   loss     = (1 / B) sum over feasible b of nll_b / T_b
//   gradient with gamma_t(s) the windowed posterior, g_sil = sum over even s, g_n = gamma_t(2n+1), g_voiced = sum_n g_n, w = scale / (B T_b):
//              d/dx[t][0] = 0
//              d/dx[t][c] = w (g_voiced softmax_{1..V-1}(x[t])[c] - sum_{n: c_n = c} g_n)        1 <= c < V
//              d/dx[t][V] = w (sigmoid(x[t][V]) - g_sil)
// The -1000 clip of the emission prep is treated as inactive (an emission that reaches it gets the gradient of the unclipped expression);
// a label whose class lies outside 1..V-1 has the constant emission -1000 and takes no part in the gradient.  Jump arcs of optional spans
// weigh a constant, so they change gamma and nothing else.
//
// Launches of one call, all on the caller's stream:
//   prep        one workgroup per clip: the frame counts as an array, skip_from compacted to [B][Lmax+1], the -1 onset / offset rows the
//               sweep wants, and per label position the chain "next position with the same class" + "first position of its class"
//   emissions   one 256-thread workgroup per (b, t) row, the row held in registers between the maximum and the sum (ONE read): the
//               reduction order and the emission formulas of emissions_from_logits_kernel (la_elementwise.hip) -- both call la_row.h's one
//               definition -- so the same bits; keeps lse_{1..V-1} (as the row's maximum and the log of the sum, apart) and x[t][V]
//   sweep       la_alignment_posteriors_windows (la_posterior.hip, through the C ABI) with gamma written to the workspace; log_z and status
//   gradient    one 1024-thread workgroup per (b, t) row: g_sil / g_voiced by a fixed-order reduction of the gamma row, then every lane
//               streams its 16-byte pieces of the row from the load to the store through registers (a 21129-wide row is 21 floats per
//               lane: one read and one write of the row).  Label columns afterwards, behind a barrier: the lane of the FIRST position of
//               a class walks the class's chain in ascending position and writes the column once -- no atomics, so the same bits every
//               time, and nothing of a clip's rows depends on its batch mates
//   finish      one thread: nll per clip and the scalar loss, clips summed in ascending order
#include "la_lattice.h"
#include "la_row.h"

namespace {

using la::lattice::waves_for_labels;

// ---- workspace ---------------------------------------------------------------------------------------------------------------------------
struct Layout {
    size_t em, row_max, logsum, xs, gamma, nfr, skip, neg1, nxt, own, occ, onp, offp, pres, skp, log_z, alpha, alpha_bytes, total;
};

// false: more than 511 labels
bool plan_layout(int64_t batch, int64_t frames, int64_t max_labels, Layout *l) {
    if (waves_for_labels((int)max_labels) > 16) return false;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (size_t)la::round_up((int64_t)bytes, 256);
        return here;
    };
    const size_t rows = (size_t)batch * (size_t)frames, per_label = (size_t)batch * (size_t)max_labels;
    l->em = take(rows * (size_t)(max_labels + 1) * 4);
    l->row_max = take(rows * 4);
    l->logsum = take(rows * 4);
    l->xs = take(rows * 4);
    l->gamma = take(rows * (size_t)(2 * max_labels + 1) * 4);
    l->nfr = take((size_t)batch * 4);
    l->skip = take((size_t)batch * (size_t)(max_labels + 1) * 4);
    l->neg1 = take(per_label * 4);
    l->nxt = take(per_label * 4);
    l->own = take(per_label * 4);
    l->occ = take(per_label * 4);
    l->onp = take(per_label * 4);
    l->offp = take(per_label * 4);
    l->pres = take(per_label * 4);
    l->skp = take((size_t)batch * (size_t)(max_labels + 1) * 4);
    l->log_z = take((size_t)batch * 8);
    l->alpha_bytes = 0;
    if (la_alignment_posteriors_windows_workspace_bytes((int32_t)batch, (int32_t)frames, (int32_t)max_labels, &l->alpha_bytes) != LA_OK) return false;
    l->alpha = take(l->alpha_bytes);
    l->total = at;
    return true;
}

// ---- prep: per clip ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void anchor_prep_kernel(const int32_t *labels, int labels_stride, const int32_t *n_labels, const int32_t *n_frames,
                                                          int frames, int max_labels, const int32_t *skip_from, int skip_stride, int32_t *nfr,
                                                          int32_t *skip_c, int32_t *neg1, int32_t *nxt, int32_t *own) {
    const int b = blockIdx.x;
    const int32_t *lab = labels + (int64_t)b * labels_stride;
    const int L = min(max(n_labels[b], 0), max_labels);
    if (threadIdx.x == 0) nfr[b] = n_frames ? n_frames[b] : frames;
    for (int n = threadIdx.x; n <= max_labels; n += 256) skip_c[(int64_t)b * (max_labels + 1) + n] = skip_from ? skip_from[(int64_t)b * skip_stride + n] : -1;
    for (int n = threadIdx.x; n < max_labels; n += 256) {
        int next = -1, first = 0;
        if (n < L) {
            const int c = lab[n];
            first = 1;
            for (int m = 0; m < n; ++m)
                if (lab[m] == c) first = 0;
            for (int m = L - 1; m > n; --m)
                if (lab[m] == c) next = m;
        }
        const int64_t at = (int64_t)b * max_labels + n;
        neg1[at] = -1;
        nxt[at] = next;
        own[at] = first;
    }
}

// ---- pass 1: compact emissions, the row's normaliser and silence logit -----------------------------------------------------------------------
// CAP > 0: the V - 1 word columns 1 .. V-1 fit into CAP registers per lane (256 CAP >= V - 1) and are read once; CAP = 0: any width, the
// second sweep of the row re-reads it (it hits L2), as emissions_from_logits_kernel does.  Same values in the same order either way.
template <int CAP>
__global__ __launch_bounds__(256) void anchor_emissions_kernel(const float *logits, int64_t bs, int64_t rs, int frames, int V, const int32_t *labels,
                                                               int labels_stride, const int32_t *n_labels, int max_labels, float *em, int64_t em_bs,
                                                               int64_t em_rs, float *max_out, float *logsum_out, float *xs_out) {
    __shared__ float red[8];
    const int row = blockIdx.x;
    const int b = row / frames, t = row % frames;
    const float *x = logits + (int64_t)b * bs + (int64_t)t * rs;
    const int tid = threadIdx.x;

    float v[CAP > 0 ? CAP : 1];
    float m = -INFINITY;
    if (CAP > 0) {
#pragma unroll
        for (int i = 0; i < CAP; ++i) {
            const int c = 1 + tid + 256 * i;
            v[i] = c < V ? x[c] : -INFINITY;
        }
#pragma unroll
        for (int i = 0; i < CAP; ++i) m = fmaxf(m, v[i]);
    } else {
        for (int c = 1 + tid; c < V; c += 256) m = fmaxf(m, x[c]);
    }
    m = la::block4_max(m, red);
    float s = 0.f;
    if (CAP > 0) {
#pragma unroll
        for (int i = 0; i < CAP; ++i) s += expf(v[i] - m);   // (a column past the row adds exp(-inf) = +0)
    } else {
        for (int c = 1 + tid; c < V; c += 256) s += expf(x[c] - m);
    }
    const float logsum = logf(la::block4_sum(s, red + 4));

    const int L = min(n_labels[b], max_labels);
    float *e = em + (int64_t)b * em_bs + (int64_t)t * em_rs;
    const int32_t *lab = labels + (int64_t)b * labels_stride;
    const float xl = x[V];
    const la::SilenceTerms sil = la::silence_terms(xl);
    if (tid == 0) {
        e[0] = la::silence_emission(sil.log_sil);
        max_out[row] = m;
        logsum_out[row] = logsum;
        xs_out[row] = xl;
    }
    for (int n = tid; n < L; n += 256) {
        const int c = lab[n];
        float val = la::kEmissionFloor;
        if (c >= 1 && c < V) val = la::voiced_emission(x[c], m, logsum, sil.log_voiced);
        e[1 + n] = val;
    }
}

// ---- pass 2: the gradient row ---------------------------------------------------------------------------------------------------------------
struct GradParams {
    const float *logits;
    int64_t bs, rs;
    float *dlogits;
    int64_t dbs, drs;
    const float *gamma;   // [batch][frames][Sg]
    const float *row_max, *logsum, *xs;   // softmax_{1..V-1}(x)[c] = exp((x[c] - row_max) - logsum): the two parts of the normaliser apart, so that
                                          // the large terms, where x[c] is close to the maximum, lose nothing to the rounding of their sum
    const int32_t *labels, *n_labels, *nfr, *status, *nxt, *own;
    int32_t labels_stride, frames, V, max_labels, batch;
    float scale;
};

constexpr int kGradThreads = 1024;
constexpr int kGradUnroll = 6;   // 16-byte pieces in flight per lane: 6 x 1024 x 4 floats cover the 21129 columns of the full vocabulary in one trip

// n floats at d, every lane of the workgroup: 16-byte stores where the address allows, single floats at the two ends
__device__ __forceinline__ void zero_row(float *d, int n, int tid) {
    const int head = min((int)((4 - (((uintptr_t)d >> 2) & 3)) & 3), n);
    const int nvec = (n - head) >> 2;
    if (tid < head) d[tid] = 0.f;
    float4 *dv = reinterpret_cast<float4 *>(d + head);
    for (int i = tid; i < nvec; i += kGradThreads) dv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int done = head + 4 * nvec;
    if (tid < n - done) d[done + tid] = 0.f;
}

__global__ __launch_bounds__(kGradThreads) void anchor_grad_kernel(GradParams p) {
    __shared__ float red[2][16];
    const int row = blockIdx.x;
    const int b = row / p.frames, t = row % p.frames;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = p.V, n = V + 1;   // columns 0 .. V
    const float *x = p.logits + (int64_t)b * p.bs + (int64_t)t * p.rs;
    float *d = p.dlogits + (int64_t)b * p.dbs + (int64_t)t * p.drs;
    const int T = p.nfr[b];
    const int L = p.n_labels[b];
    // workgroup-uniform: a clip without a path (or empty, or with a bad frame count) and the rows past a clip's end are exact zeros
    if (p.status[b] != LA_OK || t >= T || L <= 0 || L > p.max_labels) {
        zero_row(d, n, tid);
        return;
    }
    const int S = 2 * L + 1, Sg = 2 * p.max_labels + 1;
    const float *gam = p.gamma + ((int64_t)b * p.frames + t) * Sg;
    const int32_t *lab = p.labels + (int64_t)b * p.labels_stride;

    // g_sil / g_voiced: lane s holds gamma_t(s); butterfly inside the wave, then the 16 wave sums in ascending order -- a fixed order
    float gs = 0.f, gv = 0.f;
    if (tid < S) {
        const float g = gam[tid];
        if (tid & 1) {
            const int c = lab[tid >> 1];
            if (c >= 1 && c < V) gv = g;
        } else {
            gs = g;
        }
    }
    gs = la::wave_sum(gs);
    gv = la::wave_sum(gv);
    if (lane == 0) { red[0][wave] = gs; red[1][wave] = gv; }
    __syncthreads();
    float g_sil = 0.f, g_voiced = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { g_sil += red[0][i]; g_voiced += red[1][i]; }

    const float w = p.scale / ((float)p.batch * (float)T);
    const float mx = p.row_max[row], ls = p.logsum[row], xs = p.xs[row];
    const float a = w * g_voiced;
    const float d_sil = w * (1.0f / (1.0f + expf(-xs)) - g_sil);
    auto column = [&](int c, float xc) { return c == 0 ? 0.f : c == V ? d_sil : a * __expf((xc - mx) - ls); };

    if ((((uintptr_t)x ^ (uintptr_t)d) & 15) == 0) {
        // the two rows share their 16-byte phase: single floats up to the first boundary, 16-byte pieces, single floats at the end
        const int head = min((int)((4 - (((uintptr_t)x >> 2) & 3)) & 3), n);
        const int nvec = (n - head) >> 2;
        if (tid < head) d[tid] = column(tid, x[tid]);
        const float4 *xv = reinterpret_cast<const float4 *>(x + head);
        float4 *dv = reinterpret_cast<float4 *>(d + head);
        for (int i0 = tid; i0 < nvec; i0 += kGradThreads * kGradUnroll) {
            float4 v[kGradUnroll];
#pragma unroll
            for (int u = 0; u < kGradUnroll; ++u) {
                const int i = i0 + u * kGradThreads;
                if (i < nvec) v[u] = xv[i];
            }
#pragma unroll
            for (int u = 0; u < kGradUnroll; ++u) {
                const int i = i0 + u * kGradThreads;
                if (i < nvec) {
                    const int c = head + 4 * i;
                    float4 r;
                    r.x = column(c, v[u].x);
                    r.y = column(c + 1, v[u].y);
                    r.z = column(c + 2, v[u].z);
                    r.w = column(c + 3, v[u].w);
                    dv[i] = r;
                }
            }
        }
        const int done = head + 4 * nvec;
        if (tid < n - done) d[done + tid] = column(done + tid, x[done + tid]);
    } else {
        for (int c = tid; c < n; c += kGradThreads) d[c] = column(c, x[c]);
    }
    __syncthreads();   // the label columns below are written a second time, by another lane: ordered behind the row's stores

    // label columns: the lane of a class's first position sums the class's gamma in ascending position and writes the column once
    if (tid < L && p.own[(int64_t)b * p.max_labels + tid]) {
        const int c = lab[tid];
        if (c >= 1 && c < V) {
            const int32_t *nx = p.nxt + (int64_t)b * p.max_labels;
            float sum = 0.f;
            for (int m = tid; m >= 0 && m < L; m = nx[m]) sum += gam[2 * m + 1];
            d[c] = w * (g_voiced * expf((x[c] - mx) - ls) - sum);
        }
    }
}

// ---- the scalar loss ---------------------------------------------------------------------------------------------------------------------------
__global__ void anchor_finish_kernel(const double *log_z, const int32_t *status, const int32_t *nfr, int batch, double *nll, float *loss) {
    double acc = 0.0;
    for (int b = 0; b < batch; ++b) {
        if (status[b] == LA_OK) {
            const double v = -log_z[b];
            nll[b] = v;
            acc += v / (double)nfr[b];
        } else {
            nll[b] = INFINITY;
        }
    }
    loss[0] = (float)(acc / (double)batch);
}

}  // namespace

extern "C" int la_anchored_alignment_loss_workspace_bytes(int32_t batch, int32_t frames, int32_t max_labels, size_t *bytes) {
    LA_CHECK_ARG(bytes && batch > 0 && frames > 0 && max_labels > 0, "anchored_alignment_loss_workspace_bytes: bad arguments");
    Layout l;
    if (!plan_layout(batch, frames, max_labels, &l)) {
        la::set_error("anchored_alignment_loss: max_labels %d exceeds 511 (one lane per lattice state, 1024 states per workgroup)", max_labels);
        return LA_EUNSUPPORTED;
    }
    *bytes = l.total;
    return LA_OK;
}

extern "C" int la_anchored_alignment_loss(const float *logits, int64_t batch_stride, int64_t row_stride, int32_t batch, int32_t frames,
                                          int32_t vocab, const int32_t *labels, int32_t labels_stride, const int32_t *n_labels,
                                          const int32_t *n_frames, int32_t max_labels, const int32_t *skip_from, int32_t skip_stride,
                                          double skip_penalty, const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride, float scale,
                                          float *loss, double *nll, int32_t *status, float *dlogits, int64_t d_batch_stride,
                                          int64_t d_row_stride, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    LA_CHECK_ARG(logits && labels && n_labels && win_lo && win_hi, "anchored_alignment_loss: null input pointer");
    LA_CHECK_ARG(loss && nll && status, "anchored_alignment_loss: null output pointer");
    LA_CHECK_ARG(batch > 0 && frames > 0 && max_labels > 0, "anchored_alignment_loss: bad sizes");
    LA_CHECK_ARG(vocab >= 3, "anchored_alignment_loss: vocab too small (word columns 0 .. vocab-1 and the silence logit at column vocab)");
    LA_CHECK_ARG(skip_penalty >= 0.0, "anchored_alignment_loss: skip_penalty must be >= 0 (and not NaN)");
    LA_CHECK_ARG(row_stride >= (int64_t)vocab + 1 && (batch == 1 || batch_stride >= (int64_t)frames * row_stride),
                 "anchored_alignment_loss: logits strides smaller than [frames][vocab + 1]");
    LA_CHECK_ARG(!dlogits || (d_row_stride >= (int64_t)vocab + 1 && (batch == 1 || d_batch_stride >= (int64_t)frames * d_row_stride)),
                 "anchored_alignment_loss: dlogits strides smaller than [frames][vocab + 1]");
    LA_CHECK_ARG(labels_stride >= max_labels && win_stride >= 2 * (int64_t)max_labels + 1 && (!skip_from || skip_stride >= max_labels + 1),
                 "anchored_alignment_loss: strides smaller than max_labels");
    Layout l;
    if (!plan_layout(batch, frames, max_labels, &l)) {
        la::set_error("anchored_alignment_loss: max_labels %d exceeds 511", max_labels);
        return LA_EUNSUPPORTED;
    }
    LA_CHECK_ARG(workspace && workspace_bytes >= l.total, "anchored_alignment_loss: workspace too small (%zu < %zu)", workspace_bytes, l.total);
    LA_CHECK_ARG((uintptr_t)workspace % 256 == 0, "anchored_alignment_loss: workspace must be 256-byte aligned");

    unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
    auto f32 = [&](size_t at) { return reinterpret_cast<float *>(ws + at); };
    auto i32 = [&](size_t at) { return reinterpret_cast<int32_t *>(ws + at); };
    float *em = f32(l.em), *row_max = f32(l.row_max), *logsum = f32(l.logsum), *xs = f32(l.xs);
    float *gamma = dlogits ? f32(l.gamma) : nullptr;   // loss only: the sweep keeps its gamma to itself
    int32_t *nfr = i32(l.nfr), *skip_c = i32(l.skip), *neg1 = i32(l.neg1), *nxt = i32(l.nxt), *own = i32(l.own);
    double *log_z = reinterpret_cast<double *>(ws + l.log_z);
    const int rows = batch * frames;
    const int64_t em_rs = max_labels + 1, em_bs = (int64_t)frames * em_rs;
    const int64_t gamma_rs = 2 * (int64_t)max_labels + 1, gamma_bs = (int64_t)frames * gamma_rs;
    {
        la::TimerScope ts("anchored_loss_prep", stream);
        hipLaunchKernelGGL(anchor_prep_kernel, dim3(batch), dim3(256), 0, stream, labels, labels_stride, n_labels, n_frames, frames, max_labels,
                           skip_from, skip_stride, nfr, skip_c, neg1, nxt, own);
        LA_LAUNCH_CHECK();
#define LA_ANCHOR_EM(CAPV)                                                                                                                \
    hipLaunchKernelGGL((anchor_emissions_kernel<CAPV>), dim3(rows), dim3(256), 0, stream, logits, batch_stride, row_stride, frames, vocab, \
                       labels, labels_stride, n_labels, max_labels, em, em_bs, em_rs, row_max, logsum, xs)
        const int per_lane = la::cdiv(vocab - 1, 256);
        if (per_lane <= 4) LA_ANCHOR_EM(4);
        else if (per_lane <= 16) LA_ANCHOR_EM(16);
        else if (per_lane <= 88) LA_ANCHOR_EM(88);   // 21128 word columns: 83 per lane
        else LA_ANCHOR_EM(0);
#undef LA_ANCHOR_EM
        LA_LAUNCH_CHECK();
    }
    // the sum-product sweep on the windowed lattice: the caller's status array, log_z, and (with a gradient) every gamma cell
    const int rc = la_alignment_posteriors_windows(em, em_bs, em_rs, labels, labels_stride, n_labels, nfr, batch, frames, max_labels, neg1, neg1,
                                                   max_labels, 0, skip_c, max_labels + 1, skip_penalty, win_lo, win_hi, win_stride, f32(l.occ),
                                                   f32(l.onp), f32(l.offp), f32(l.pres), f32(l.skp), log_z, status, gamma, gamma_bs, gamma_rs,
                                                   ws + l.alpha, l.alpha_bytes, stream_);
    if (rc != LA_OK) return rc;
    if (dlogits) {
        GradParams g{};
        g.logits = logits, g.bs = batch_stride, g.rs = row_stride;
        g.dlogits = dlogits, g.dbs = d_batch_stride, g.drs = d_row_stride;
        g.gamma = gamma, g.row_max = row_max, g.logsum = logsum, g.xs = xs;
        g.labels = labels, g.n_labels = n_labels, g.nfr = nfr, g.status = status, g.nxt = nxt, g.own = own;
        g.labels_stride = labels_stride, g.frames = frames, g.V = vocab, g.max_labels = max_labels, g.batch = batch;
        g.scale = scale;
        la::TimerScope ts("anchored_loss_grad", stream, 8.0 * (double)rows * (double)(vocab + 1));
        hipLaunchKernelGGL(anchor_grad_kernel, dim3(rows), dim3(kGradThreads), 0, stream, g);
        LA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(anchor_finish_kernel, dim3(1), dim3(1), 0, stream, log_z, status, nfr, batch, nll, loss);
    LA_LAUNCH_CHECK();
    return LA_OK;
}
