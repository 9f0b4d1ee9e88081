// la_readings.hip -- pronunciation alternatives (DESIGN.md "Pronunciation alternatives"): a label position may have several readings
// (class ids).  The emissions of every reading come from the existing head / prep on the EXPANDED label list; the two kernels here sit
// in front of and behind the lattice:
//   * la_emissions_merge_readings folds the expanded compact matrix em_x into the matrix the lattice reads: a position's column is the
//     log of the sum of its readings' probabilities (the merged class);
//   * la_reading_scores sums every expanded column over the segment the DP gave its position and names the reading with the largest sum.
// Both are memory-bound data movement with a little float64 arithmetic: no LDS, no atomics, no dependence between clips, so a clip's
// bits are the same alone and in a batch, and two calls agree bit for bit.
#include <math.h>

#include "la_row.h"

namespace {

constexpr int kMaxColumns = 4095;      // the widest lattice (la_viterbi.hip: 8192 states per workgroup) and the widest expanded matrix
constexpr int kColLanes = 64;          // merge: one wave across neighbouring output columns ...
constexpr int kRowGroups = 4;          //        ... times four row groups per 256-thread workgroup
constexpr int kRowTile = 32;           //        rows per workgroup: a thread owns one output column for kRowTile / kRowGroups rows

// The CSR pair of output column c >= 1 (position n = c - 1) of one clip, clamped into 0 .. max_columns so that a malformed row can never
// read outside the expanded row (the host cannot check device data): -> first expanded column index j0 and the count A (0 = empty group).
__device__ __forceinline__ void group_of(const int32_t *alt, int n, int max_columns, int &j0, int &A) {
    int s = alt[n], e = alt[n + 1];
    s = s < 0 ? 0 : (s > max_columns ? max_columns : s);
    e = e < s ? s : (e > max_columns ? max_columns : e);
    j0 = s;
    A = e - s;
}

// em[b][t][0] = em_x[b][t][0]; em[b][t][1+n] = the fold of em_x[b][t][1 + alt[n] .. alt[n+1]] (one reading: the value itself, bit for bit).
// Scalar 4-byte accesses only: row starts and group starts have no alignment that could be proven.
__global__ __launch_bounds__(kColLanes *kRowGroups) void merge_readings_kernel(
    const float *__restrict__ em_x, int64_t xbs, int64_t xrs, const int32_t *__restrict__ alt_start, int alt_stride,
    const int32_t *__restrict__ n_labels, const int32_t *__restrict__ n_frames, int max_frames, int max_labels, int max_columns,
    float *__restrict__ em, int64_t ebs, int64_t ers) {
    const int b = blockIdx.z;
    int L = n_labels[b], T = n_frames[b];
    L = L < 0 ? 0 : (L > max_labels ? max_labels : L);
    T = T < 0 ? 0 : (T > max_frames ? max_frames : T);
    const int c = blockIdx.x * kColLanes + (threadIdx.x & (kColLanes - 1));       // output column: 0 = silence, 1 + n = position n
    const int t0 = blockIdx.y * kRowTile + (threadIdx.x / kColLanes);
    if (c > L || t0 >= T) return;
    int j0 = 0, A = 1;                                                             // silence: expanded column 0, one "reading"
    if (c > 0) {
        group_of(alt_start + (int64_t)b * alt_stride, c - 1, max_columns, j0, A);
        j0 += 1;
    }
    const int t_end = min(T, (int)(blockIdx.y + 1) * kRowTile);
    const float *xb = em_x + (int64_t)b * xbs + j0;
    float *eb = em + (int64_t)b * ebs + c;
    for (int t = t0; t < t_end; t += kRowGroups) {
        const float *x = xb + (int64_t)t * xrs;
        float r;
        if (A == 1) {
            r = x[0];
        } else {
            float m = -INFINITY;
            for (int a = 0; a < A; ++a) m = fmaxf(m, x[a]);
            if (m == -INFINITY) {                                                  // every reading impossible (or an empty group)
                r = -INFINITY;
            } else {
                double sum = 0.0;                                                  // float64, ascending a, rounded once
                for (int a = 0; a < A; ++a) sum += exp((double)x[a] - (double)m);
                r = (float)((double)m + log(sum));
            }
        }
        eb[(int64_t)t * ers] = r;
    }
}

// One workgroup per clip.  Phase 1, one lane per expanded column j: col_score[j] = the float64 sum of em_x[t][1+j] over t ascending in
// [onset, offset) of the column's position (0 for a skipped position).  Phase 2, one lane per position: the smallest reading index with
// the largest score, as a class-free index 0 .. A-1 (-1 for a skipped position).  The workgroup's own global stores are visible to it
// after the barrier.
__global__ __launch_bounds__(256) void reading_scores_kernel(
    const float *__restrict__ em_x, int64_t xbs, int64_t xrs, const int32_t *__restrict__ alt_start, int alt_stride,
    const int32_t *__restrict__ n_labels, const int32_t *__restrict__ onset, const int32_t *__restrict__ offset, int out_stride,
    int max_frames, int max_labels, int max_columns, double *col_score, int col_stride, int32_t *__restrict__ reading,
    int reading_stride) {
    const int b = blockIdx.x;
    int L = n_labels[b];
    L = L < 0 ? 0 : (L > max_labels ? max_labels : L);
    const int32_t *alt = alt_start + (int64_t)b * alt_stride;
    const int32_t *on = onset + (int64_t)b * out_stride, *off = offset + (int64_t)b * out_stride;
    double *score = col_score + (int64_t)b * col_stride;
    int n_cols = 0, unused = 0;
    if (L > 0) {
        group_of(alt, L - 1, max_columns, n_cols, unused);
        n_cols += unused;                                                          // = alt[L], clamped
    }
    const float *xb = em_x + (int64_t)b * xbs + 1;
    for (int j = threadIdx.x; j < n_cols; j += 256) {
        int lo = 0, hi = L - 1;                                                    // the position n with alt[n] <= j < alt[n+1]
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (alt[mid] <= j) lo = mid; else hi = mid - 1;
        }
        int t = on[lo], u = off[lo];
        double s = 0.0;
        if (t >= 0) {
            u = u > max_frames ? max_frames : u;
            for (; t < u; ++t) s += (double)xb[(int64_t)t * xrs + j];
        }
        score[j] = s;
    }
    __syncthreads();
    for (int n = threadIdx.x; n < L; n += 256) {
        int best = -1;
        if (on[n] >= 0) {
            int j0, A;
            group_of(alt, n, max_columns, j0, A);
            double top = 0.0;
            for (int a = 0; a < A; ++a) {
                const double s = score[j0 + a];
                if (best < 0 || s > top) { best = a; top = s; }
            }
        }
        reading[(int64_t)b * reading_stride + n] = best;
    }
}

// the argument errors the two entries share, under the entry's name
int check_common(const char *who, const void *em_x, const void *alt_start, const void *n_labels, int64_t xbs, int64_t xrs, int alt_stride,
                 int batch, int max_frames, int max_labels, int max_columns) {
    LA_CHECK_ARG(em_x && alt_start && n_labels, "%s: null pointer", who);
    LA_CHECK_ARG(batch > 0 && max_frames > 0 && max_labels > 0, "%s: bad sizes (batch, max_frames and max_labels must be > 0)", who);
    if (max_labels > kMaxColumns || max_columns > kMaxColumns) {
        la::set_error("%s: max_labels %d / max_columns %d exceed 4095", who, max_labels, max_columns);
        return LA_EUNSUPPORTED;
    }
    LA_CHECK_ARG(max_columns >= max_labels, "%s: max_columns %d < max_labels %d (every position has at least one reading)", who, max_columns,
                 max_labels);
    LA_CHECK_ARG(xrs >= (int64_t)max_columns + 1 && alt_stride >= max_labels + 1 &&
                     (batch == 1 || xbs >= (int64_t)(max_frames - 1) * xrs + max_columns + 1),
                 "%s: strides smaller than the widths (em_x rows hold max_columns + 1, alt_start rows max_labels + 1 entries)", who);
    return LA_OK;
}

}  // namespace

extern "C" int la_emissions_merge_readings(const float *em_x, int64_t emx_batch_stride, int64_t emx_row_stride, const int32_t *alt_start,
                                           int32_t alt_stride, const int32_t *n_labels, const int32_t *n_frames, int32_t batch,
                                           int32_t max_frames, int32_t max_labels, int32_t max_columns, float *em,
                                           int64_t em_batch_stride, int64_t em_row_stride, void *stream_) {
    static const char who[] = "emissions_merge_readings";
    hipStream_t stream = (hipStream_t)stream_;
    LA_CHECK_ARG(n_frames && em, "%s: null pointer", who);
    if (const int rc = check_common(who, em_x, alt_start, n_labels, emx_batch_stride, emx_row_stride, alt_stride, batch, max_frames,
                                    max_labels, max_columns))
        return rc;
    LA_CHECK_ARG(em_row_stride >= (int64_t)max_labels + 1 &&
                     (batch == 1 || em_batch_stride >= (int64_t)(max_frames - 1) * em_row_stride + max_labels + 1),
                 "%s: strides smaller than the widths (em rows hold max_labels + 1 entries)", who);
    la::TimerScope ts(who, stream);
    const dim3 grid((max_labels + 1 + kColLanes - 1) / kColLanes, (max_frames + kRowTile - 1) / kRowTile, batch);
    hipLaunchKernelGGL(merge_readings_kernel, grid, dim3(kColLanes * kRowGroups), 0, stream, em_x, emx_batch_stride, emx_row_stride,
                       alt_start, alt_stride, n_labels, n_frames, max_frames, max_labels, max_columns, em, em_batch_stride, em_row_stride);
    LA_LAUNCH_CHECK();
    return LA_OK;
}

extern "C" int la_reading_scores(const float *em_x, int64_t emx_batch_stride, int64_t emx_row_stride, const int32_t *alt_start,
                                 int32_t alt_stride, const int32_t *n_labels, const int32_t *onset, const int32_t *offset,
                                 int32_t out_stride, int32_t batch, int32_t max_frames, int32_t max_labels, int32_t max_columns,
                                 double *col_score, int32_t col_stride, int32_t *reading, int32_t reading_stride, void *stream_) {
    static const char who[] = "reading_scores";
    hipStream_t stream = (hipStream_t)stream_;
    LA_CHECK_ARG(onset && offset && col_score && reading, "%s: null pointer", who);
    if (const int rc = check_common(who, em_x, alt_start, n_labels, emx_batch_stride, emx_row_stride, alt_stride, batch, max_frames,
                                    max_labels, max_columns))
        return rc;
    LA_CHECK_ARG(out_stride >= max_labels && reading_stride >= max_labels && col_stride >= max_columns,
                 "%s: strides smaller than the widths (onset / offset / reading rows hold max_labels, col_score rows max_columns entries)", who);
    la::TimerScope ts(who, stream);
    hipLaunchKernelGGL(reading_scores_kernel, dim3(batch), dim3(256), 0, stream, em_x, emx_batch_stride, emx_row_stride, alt_start,
                       alt_stride, n_labels, onset, offset, out_stride, max_frames, max_labels, max_columns, col_score, col_stride, reading,
                       reading_stride);
    LA_LAUNCH_CHECK();
    return LA_OK;
}
