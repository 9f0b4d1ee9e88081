// la_offsheet.hip -- off-sheet slots (DESIGN.md "Off-sheet slots"): a label position of the lattice that stands for "singing the sheet does
// not have".  Its emission column holds log P(frame is not silence) - penalty, a function of column 0 of the compact emission matrix
// alone (both emission providers leave log P(silence), clamped at -1000, there in both variants), so one kernel serves every route:
//   v   = log(-expm1((double)em[b][t][0])) - penalty          float64
//   out = v > -1000.0 ? (float)v : -1000.0f                   rounded once; v NaN or -inf (em NaN or >= 0): the floor
//   em[b][t][1 + x] = out  for every slot column x of clip b and every t < n_frames[b]
// In place, element-granular scatter stores, the float64 transcendentals once per row.  No atomics, nothing shared between clips: a
// clip's bits are the same alone and in a batch, and two calls agree bit for bit.
#include <math.h>

#include "la_row.h"

namespace {

constexpr int kMaxLabels = 4095;       // the widest lattice (la_viterbi.hip)
constexpr int kThreads = 256;
constexpr int kTileRows = 64;          // the slot-major form: rows per workgroup, their values staged in LDS

__device__ __forceinline__ float slot_value(float silence, double penalty) {
    const double v = log(-expm1((double)silence)) - penalty;
    return v > (double)la::kEmissionFloor ? (float)v : la::kEmissionFloor;
}

__device__ __forceinline__ int clamped(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

#ifdef LA_EXPERIMENTS
// Frame-major, the other lane mapping that was measured (profiles/offsheet.txt: no faster at either shape, the same bits): a lane owns one
// frame, evaluates its value once and walks the clip's slots (the slot list is wave-uniform: scalar loads).  In the experiment build
// only, for tools/offsheet_bench.py; the shipped library has the one form below.
__global__ __launch_bounds__(kThreads) void offsheet_rows_kernel(
    float *__restrict__ em, int64_t ebs, int64_t ers, const int32_t *__restrict__ slot_cols, int slot_stride,
    const int32_t *__restrict__ n_slots, const int32_t *__restrict__ n_frames, int max_frames, int max_labels, int max_slots,
    double penalty) {
    const int b = blockIdx.y;
    const int S = clamped(n_slots[b], max_slots), T = clamped(n_frames[b], max_frames);
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (S == 0 || t >= T) return;
    float *row = em + (int64_t)b * ebs + (int64_t)t * ers;
    const float out = slot_value(row[0], penalty);
    const int32_t *cols = slot_cols + (int64_t)b * slot_stride;
    for (int i = 0; i < S; ++i) {
        const int x = cols[i];
        if (x >= 0 && x < max_labels) row[1 + x] = out;
    }
}
#endif

// Slot-major: the workgroup's first kTileRows lanes evaluate one row each into LDS; then every lane takes
// (row, slot) pairs, the slots of one row on neighbouring lanes.
__global__ __launch_bounds__(kThreads) void offsheet_slots_kernel(
    float *__restrict__ em, int64_t ebs, int64_t ers, const int32_t *__restrict__ slot_cols, int slot_stride,
    const int32_t *__restrict__ n_slots, const int32_t *__restrict__ n_frames, int max_frames, int max_labels, int max_slots,
    double penalty) {
    __shared__ float value[kTileRows];
    const int b = blockIdx.y;
    const int S = clamped(n_slots[b], max_slots), T = clamped(n_frames[b], max_frames);
    const int t0 = blockIdx.x * kTileRows;
    if (S == 0 || t0 >= T) return;                                   // uniform over the workgroup: no lane waits at the barrier below
    const int rows = min(kTileRows, T - t0);
    float *base = em + (int64_t)b * ebs + (int64_t)t0 * ers;
    if ((int)threadIdx.x < rows) value[threadIdx.x] = slot_value(base[(int64_t)threadIdx.x * ers], penalty);
    __syncthreads();
    const int32_t *cols = slot_cols + (int64_t)b * slot_stride;
    for (int item = threadIdx.x; item < rows * S; item += kThreads) {
        const int r = item / S, x = cols[item - r * S];
        if (x >= 0 && x < max_labels) base[(int64_t)r * ers + 1 + x] = value[r];
    }
}

}  // namespace

extern "C" int la_emissions_offsheet_columns(float *em, int64_t em_batch_stride, int64_t em_row_stride, const int32_t *slot_cols,
                                             int32_t slot_stride, const int32_t *n_slots, const int32_t *n_frames, int32_t batch,
                                             int32_t max_frames, int32_t max_labels, int32_t max_slots, double penalty, void *stream_) {
    static const char who[] = "emissions_offsheet_columns";
    hipStream_t stream = (hipStream_t)stream_;
    LA_CHECK_ARG(em && slot_cols && n_slots && n_frames, "%s: null pointer", who);
    LA_CHECK_ARG(batch > 0 && max_frames > 0 && max_labels > 0 && max_slots > 0,
                 "%s: bad sizes (batch, max_frames, max_labels and max_slots must be > 0)", who);
    LA_CHECK_ARG(penalty >= 0.0, "%s: penalty must be >= 0 (and not NaN)", who);
    if (max_labels > kMaxLabels || batch > 65535) {
        la::set_error("%s: max_labels %d exceeds 4095 (or more than 65535 clips)", who, max_labels);
        return LA_EUNSUPPORTED;
    }
    LA_CHECK_ARG(em_row_stride >= (int64_t)max_labels + 1 && slot_stride >= max_slots,
                 "%s: strides smaller than the widths (em rows hold max_labels + 1, slot_cols rows max_slots entries)", who);
    la::TimerScope ts(who, stream);
#ifdef LA_EXPERIMENTS
    const char *form = la::dev_env("LA_OFFSHEET_FORM");          // "rows": the frame-major form (developer switch, re-read per launch)
    if (form && strcmp(form, "rows") == 0) {
        hipLaunchKernelGGL(offsheet_rows_kernel, dim3(la::cdiv(max_frames, kThreads), batch), dim3(kThreads), 0, stream, em,
                           em_batch_stride, em_row_stride, slot_cols, slot_stride, n_slots, n_frames, max_frames, max_labels, max_slots,
                           penalty);
        LA_LAUNCH_CHECK();
        return LA_OK;
    }
#endif
    hipLaunchKernelGGL(offsheet_slots_kernel, dim3(la::cdiv(max_frames, kTileRows), batch), dim3(kThreads), 0, stream, em, em_batch_stride,
                       em_row_stride, slot_cols, slot_stride, n_slots, n_frames, max_frames, max_labels, max_slots, penalty);
    LA_LAUNCH_CHECK();
    return LA_OK;
}
