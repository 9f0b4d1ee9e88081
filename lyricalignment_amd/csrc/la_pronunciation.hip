// la_pronunciation.hip -- pronunciation scores (DESIGN.md "Pronunciation scores"): was the sheet's character the one that was sung?
// The lattice forces every state onto its sheet class, so a wrong character still gets a confident-looking segment.  After the DP,
// la_segment_class_scores sums the emissions of EVERY candidate class (all 402 syllables, say) over the segment the DP gave a position,
// ranks the position's own class among them and names the top few classes heard there: "goodness of pronunciation".
//   * one workgroup per (clip, position); lane tid owns the candidate columns tid + 256 i, so a frame row is read coalesced;
//   * two groups of kRowsAhead rows of independent loads are in flight while rows are added in ascending t: the order of the float64 sum
//     is fixed (sequential, as la_reading_scores'), only the loads run ahead;
//   * the position's n_cand sums go to LDS (8 n_cand bytes, at most 32760), where top_k rounds of a wave-then-workgroup arg-max on the
//     key (score, -column) select; the rank of the own class is a counted compare.
// Segments of one clip are disjoint, so a call reads every emission at most once.  No atomics, nothing shared between workgroups: a
// position's bits are the same alone and in a batch, and two calls agree bit for bit.
#include <math.h>

#include "la_row.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kColsPerThread = 2;                       // columns a lane sums at a time: tid and tid + 256 of the chunk
constexpr int kChunk = kThreads * kColsPerThread;       // candidate columns per pass over the segment's rows
constexpr int kRowsAhead = 8;                           // rows per group of loads; two groups in flight: up to 32 loads per lane
constexpr int kMaxCand = 4095;
constexpr int kMaxLabels = 4095;
constexpr int kMaxTopK = 16;

// (sa, ja) comes before (sb, jb) in the ranking: the larger sum, on a tie the smaller column; j < 0 = no candidate
__device__ __forceinline__ bool before(double sa, int ja, double sb, int jb) {
    return ja >= 0 && (jb < 0 || sa > sb || (sa == sb && ja < jb));
}

// xor butterflies 32 -> 1 on the key: the ranking is a total order, so every lane ends with the wave's first candidate
__device__ __forceinline__ void wave_first(double &s, int &j) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double os = __shfl_xor(s, m);
        const int oj = __shfl_xor(j, m);
        if (before(os, oj, s, j)) { s = os; j = oj; }
    }
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(kThreads) void segment_class_scores_kernel(
    const float *__restrict__ em_c, int64_t ebs, int64_t ers, const int32_t *__restrict__ n_labels, const int32_t *__restrict__ onset,
    const int32_t *__restrict__ offset, int out_stride, const int32_t *__restrict__ own_col, int own_stride, int max_frames, int max_labels,
    int n_cand, int top_k, double *__restrict__ seg_score, int64_t sbs, int64_t srs, int32_t *__restrict__ top_col,
    double *__restrict__ top_score, int top_stride, double *__restrict__ own_score, int32_t *__restrict__ own_rank,
    int32_t *__restrict__ n_seg_frames) {
    extern __shared__ __align__(16) double score[];                                // [n_cand]: the position's sums
    __shared__ double red_s[2][kWaves];
    __shared__ int red_j[2][kWaves];
    const int n = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    int L = n_labels[b];
    L = L < 0 ? 0 : (L > max_labels ? max_labels : L);
    if (n >= L) return;                                                            // beyond the clip's labels nothing is written
    const int64_t o = (int64_t)b * out_stride + n;
    int32_t *tc = top_col + ((int64_t)b * max_labels + n) * top_stride;
    double *ts = top_score + ((int64_t)b * max_labels + n) * top_stride;
    double *seg = seg_score ? seg_score + (int64_t)b * sbs + (int64_t)n * srs : nullptr;
    int t0 = onset[o], t1 = offset[o];
    if (t0 < 0) {                                                                  // a skipped position
        for (int k = tid; k < top_k; k += kThreads) { tc[k] = -1; ts[k] = 0.0; }
        if (seg)
            for (int j = tid; j < n_cand; j += kThreads) seg[j] = 0.0;
        if (tid == 0) { own_score[o] = 0.0; own_rank[o] = -1; n_seg_frames[o] = 0; }
        return;
    }
    t0 = t0 > max_frames ? max_frames : t0;                                        // device data: a malformed row reads nothing outside its clip
    t1 = t1 > max_frames ? max_frames : t1;
    t1 = t1 < t0 ? t0 : t1;
    const float *eb = em_c + (int64_t)b * ebs;
    for (int c0 = 0; c0 < n_cand; c0 += kChunk) {
        const int j0 = c0 + tid, j1 = j0 + kThreads;
        const bool h0 = j0 < n_cand, h1 = j1 < n_cand;
        double s0 = 0.0, s1 = 0.0;
        // Two groups of kRowsAhead rows are in flight: while group A is added, group B's loads are outstanding, and A's next loads are
        // issued before B is added.  Rows at or beyond t1 are neither loaded nor added (workgroup-uniform), so a short segment costs one
        // group of independent loads, not a chain of one load per add.
        float a0[kRowsAhead], a1[kRowsAhead], b0[kRowsAhead], b1[kRowsAhead];
        auto load = [&](float *v0, float *v1, int t) {
            const float *p = eb + (int64_t)t * ers;
#pragma unroll
            for (int r = 0; r < kRowsAhead; ++r) {
                const bool row = t + r < t1;
                v0[r] = (row && h0) ? p[(int64_t)r * ers + j0] : 0.0f;
                v1[r] = (row && h1) ? p[(int64_t)r * ers + j1] : 0.0f;
            }
        };
        auto add = [&](const float *v0, const float *v1, int t) {
#pragma unroll
            for (int r = 0; r < kRowsAhead; ++r)                                   // ascending t
                if (t + r < t1) {
                    s0 += (double)v0[r];
                    s1 += (double)v1[r];
                }
        };
        load(a0, a1, t0);
        for (int t = t0; t < t1; t += 2 * kRowsAhead) {
            load(b0, b1, t + kRowsAhead);
            add(a0, a1, t);
            load(a0, a1, t + 2 * kRowsAhead);
            add(b0, b1, t + kRowsAhead);
        }
        if (h0) { score[j0] = s0; if (seg) seg[j0] = s0; }
        if (h1) { score[j1] = s1; if (seg) seg[j1] = s1; }
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    // the own class: its sum, and how many candidates come before it
    int oc = own_col[(int64_t)b * own_stride + n];
    oc = (oc < 0 || oc >= n_cand) ? -1 : oc;
    int rank = -1;
    double own = 0.0;
    if (oc >= 0) {                                                                 // workgroup-uniform
        own = score[oc];
        int cnt = 0;
        for (int j = tid; j < n_cand; j += kThreads) cnt += before(score[j], j, own, oc) ? 1 : 0;
        cnt = wave_sum(cnt);
        if (lane == 0) red_j[1][wave] = cnt;                                       // (buffer 1: round 0 of the selection writes buffer 0)
        __syncthreads();
        rank = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) rank += red_j[1][w];
    }
    if (tid == 0) { own_score[o] = own; own_rank[o] = rank; n_seg_frames[o] = t1 - t0; }

    // top_k rounds: the first candidate behind the previous pick.  (No marking: -inf is an ordinary sum.)  One barrier per round: the
    // reduction buffers alternate, and a wave that writes buffer k & 1 again in round k + 2 has passed round k + 1's barrier, which
    // every wave reaches only after its reads of round k.
    double ps = 0.0;
    int pj = -1;
    for (int k = 0; k < top_k; ++k) {
        double bs = 0.0;
        int bj = -1;
        for (int j = tid; j < n_cand; j += kThreads) {
            const double s = score[j];
            if ((pj < 0 || before(ps, pj, s, j)) && before(s, j, bs, bj)) { bs = s; bj = j; }
        }
        wave_first(bs, bj);
        if (lane == 0) { red_s[k & 1][wave] = bs; red_j[k & 1][wave] = bj; }
        __syncthreads();
        bs = red_s[k & 1][0];
        bj = red_j[k & 1][0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            const double s = red_s[k & 1][w];
            const int j = red_j[k & 1][w];
            if (before(s, j, bs, bj)) { bs = s; bj = j; }
        }
        if (bj < 0) {                                                              // top_k > n_cand: the trailing entries
            if (tid == 0)
                for (int r = k; r < top_k; ++r) { tc[r] = -1; ts[r] = -INFINITY; }
            break;                                                                 // workgroup-uniform
        }
        if (tid == 0) { tc[k] = bj; ts[k] = bs; }
        ps = bs;
        pj = bj;
    }
}

}  // namespace

extern "C" int la_segment_class_scores(const float *em_c, int64_t emc_batch_stride, int64_t emc_row_stride, const int32_t *n_labels,
                                       const int32_t *onset, const int32_t *offset, int32_t out_stride, const int32_t *own_col,
                                       int32_t own_stride, int32_t batch, int32_t max_frames, int32_t max_labels, int32_t n_cand,
                                       int32_t top_k, double *seg_score, int64_t seg_batch_stride, int64_t seg_row_stride,
                                       int32_t *top_col, double *top_score, int32_t top_stride, double *own_score, int32_t *own_rank,
                                       int32_t *n_seg_frames, void *stream_) {
    static const char who[] = "segment_class_scores";
    hipStream_t stream = (hipStream_t)stream_;
    LA_CHECK_ARG(em_c && n_labels && onset && offset && own_col && top_col && top_score && own_score && own_rank && n_seg_frames,
                 "%s: null pointer", who);
    LA_CHECK_ARG(batch > 0 && max_frames > 0 && max_labels > 0 && n_cand > 0 && top_k > 0,
                 "%s: bad sizes (batch, max_frames, max_labels, n_cand and top_k must be > 0)", who);
    if (max_labels > kMaxLabels || n_cand > kMaxCand || top_k > kMaxTopK) {
        la::set_error("%s: max_labels %d / n_cand %d exceed 4095 or top_k %d exceeds 16", who, max_labels, n_cand, top_k);
        return LA_EUNSUPPORTED;
    }
    if (batch > 65535) {
        la::set_error("%s: batch %d exceeds 65535 (one grid row per clip)", who, batch);
        return LA_EUNSUPPORTED;
    }
    LA_CHECK_ARG(emc_row_stride >= (int64_t)n_cand && (batch == 1 || emc_batch_stride >= (int64_t)(max_frames - 1) * emc_row_stride + n_cand) &&
                     out_stride >= max_labels && own_stride >= max_labels && top_stride >= top_k &&
                     (!seg_score || (seg_row_stride >= (int64_t)n_cand &&
                                     (batch == 1 || seg_batch_stride >= (int64_t)(max_labels - 1) * seg_row_stride + n_cand))),
                 "%s: strides smaller than the widths (em_c / seg_score rows hold n_cand, onset / offset / own_col / own_score / own_rank / "
                 "n_seg_frames rows max_labels, top_col / top_score rows top_k entries)", who);
    la::TimerScope ts(who, stream);
    hipLaunchKernelGGL(segment_class_scores_kernel, dim3(max_labels, batch), dim3(kThreads), (size_t)n_cand * sizeof(double), stream, em_c,
                       emc_batch_stride, emc_row_stride, n_labels, onset, offset, out_stride, own_col, own_stride, max_frames, max_labels,
                       n_cand, top_k, seg_score, seg_batch_stride, seg_row_stride, top_col, top_score, top_stride, own_score, own_rank,
                       n_seg_frames);
    LA_LAUNCH_CHECK();
    return LA_OK;
}
