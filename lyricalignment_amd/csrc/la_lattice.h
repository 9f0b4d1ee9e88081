// la_lattice.h -- what the kernels that sweep the alignment lattice (S = 2L+1 states, one lane per state, row by row) have in
// common: la_viterbi.hip (max-product), la_posterior.hip and the CTC lattice of la_loss.hip (sum-product).  Device helpers for
// the neighbour exchange inside one wave64, the span-source rule and the log-sum-exp of a step; on the host the wave count of a label count, the face of
// an entry point (plain, optional spans, frame windows) with its names, and the description of the lattice with its argument checks.
// la_lattice_tile.h, on top of this header, is the form of a kernel with R states per thread and the host path of its entry.
#pragma once

#include "la_common.h"

namespace la {
namespace lattice {

constexpr size_t kLdsBudget = 160 * 1024 - 1024;  // dynamic LDS a lattice kernel may ask for (the CU has 160 KiB)

// one lane per state: the smallest power-of-two wave count that holds 2 * max_labels + 1 states (a workgroup has at most 16)
inline int waves_for_labels(int max_labels) {
    const int S = 2 * max_labels + 1;
    int nw = 1;
    while (nw * 64 < S) nw *= 2;
    return nw;
}

// ---- host side: what the entry points of la_viterbi.hip and la_posterior.hip share ------------------------------------------------
// The face of a call: which lattice it sweeps.  Windows is Spans plus a frame window per state (a null skip_from = no span anywhere);
// both run the SPANS instantiations.  Decided by the extern "C" entry point, nowhere else.
enum class Face { Plain, Spans, Windows };
enum class Sweep { Dp, Posteriors };

// entry: the "who" of an entry point's messages; query: of its workspace query (and of the label-limit message); timer: its TimerScope
struct FaceNames {
    const char *entry, *query, *timer;
};
inline const FaceNames &face_names(Sweep sweep, Face face) {
    static const FaceNames table[2][3] = {
        {{"viterbi_batch", "viterbi", "viterbi"},
         {"viterbi_spans_batch", "viterbi_spans", "viterbi_spans"},
         {"viterbi_windows_batch", "viterbi_windows", "viterbi_windows"}},
        {{"alignment_posteriors", "alignment_posteriors", "posterior"},
         {"alignment_posteriors_spans", "alignment_posteriors_spans", "posterior_spans"},
         {"alignment_posteriors_windows", "alignment_posteriors_windows", "posterior_windows"}}};
    return table[(int)sweep][(int)face];
}

// The caller's description of the lattice, read by every kernel that sweeps it.  VitParams and PostParams derive from it (the kernels
// write p.em, p.skip_from, ...) and add their outputs and workspace.  Filled by name: what a face does not have stays zero.
struct LatticeIn {
    const float *em;
    int64_t em_bs, em_rs;
    const int32_t *labels;
    int32_t labels_stride;
    const int32_t *n_labels;
    const int32_t *n_frames;
    int32_t max_frames, max_labels;
    // optional spans (SPANS instantiations only)
    const int32_t *skip_from;
    int32_t skip_stride;
    double penalty;
    // per-state frame windows (WIN instantiations only): [batch][win_stride], entries 0 .. 2 L_b of row b are read
    const int32_t *win_lo, *win_hi;
    int32_t win_stride;

    void set_inputs(const float *em_, int64_t em_batch_stride, int64_t em_row_stride, const int32_t *labels_, int32_t labels_stride_,
                    const int32_t *n_labels_, const int32_t *n_frames_, int32_t max_frames_, int32_t max_labels_) {
        em = em_, em_bs = em_batch_stride, em_rs = em_row_stride;
        labels = labels_, labels_stride = labels_stride_;
        n_labels = n_labels_, n_frames = n_frames_;
        max_frames = max_frames_, max_labels = max_labels_;
    }
    void set_spans(const int32_t *skip_from_, int32_t skip_stride_, double skip_penalty) {
        skip_from = skip_from_, skip_stride = skip_stride_, penalty = skip_penalty;
    }
    void set_windows(const int32_t *lo, const int32_t *hi, int32_t stride) { win_lo = lo, win_hi = hi, win_stride = stride; }

    // the argument checks of a face, for the entry points to report under their own names and in their own order
    bool inputs_present(Face face) const {
        return em && labels && n_labels && n_frames && (face != Face::Spans || skip_from) && (face != Face::Windows || (win_lo && win_hi));
    }
    bool sizes_ok(int32_t batch) const { return batch > 0 && max_frames > 0 && max_labels > 0; }
    bool penalty_ok(Face face) const { return face == Face::Plain || penalty >= 0.0; }  // false for NaN
    // out_stride: the row pitch of the entry's [batch][max_labels] arrays.  skip_stride counts where a skip_from is read, and for the
    // posteriors with a null one too (pitch_of_output: it is the row pitch of span_skip_prob).
    bool strides_ok(Face face, int32_t out_stride, bool pitch_of_output) const {
        return em_rs >= max_labels + 1 && out_stride >= max_labels && labels_stride >= max_labels &&
               (face == Face::Plain || !(skip_from || pitch_of_output) || skip_stride >= max_labels + 1) &&
               (face != Face::Windows || win_stride >= 2 * max_labels + 1);
    }
};

// DPP wave_shr:1 / wave_shl:1 -- across the whole wave64 (gfx9 family); the lane without a neighbour receives `fill`
__device__ __forceinline__ double wave_shr1(double x, double fill) {  // lane i <- lane i-1, lane 0 <- fill
    const int lo = __double2loint(x), hi = __double2hiint(x), flo = __double2loint(fill), fhi = __double2hiint(fill);
    const int rlo = __builtin_amdgcn_update_dpp(flo, lo, 0x138, 0xf, 0xf, false);
    const int rhi = __builtin_amdgcn_update_dpp(fhi, hi, 0x138, 0xf, 0xf, false);
    return __hiloint2double(rhi, rlo);
}
__device__ __forceinline__ double wave_shl1(double x, double fill) {  // lane i <- lane i+1, lane 63 <- fill
    const int lo = __double2loint(x), hi = __double2hiint(x), flo = __double2loint(fill), fhi = __double2hiint(fill);
    const int rlo = __builtin_amdgcn_update_dpp(flo, lo, 0x130, 0xf, 0xf, false);
    const int rhi = __builtin_amdgcn_update_dpp(fhi, hi, 0x130, 0xf, 0xf, false);
    return __hiloint2double(rhi, rlo);
}
// lane i receives x of lane (byte_addr / 4); byte_addr is always a lane of this wave
__device__ __forceinline__ double wave_gather(double x, int byte_addr) {
    const int lo = __builtin_amdgcn_ds_bpermute(byte_addr, __double2loint(x));
    const int hi = __builtin_amdgcn_ds_bpermute(byte_addr, __double2hiint(x));
    return __hiloint2double(hi, lo);
}
// lane i receives x of the lane that the DPP control CTRL names (a permutation inside a row of 16 lanes: every lane has a source)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
    const int lo = __double2loint(x), hi = __double2hiint(x);
    return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false), __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false));
}
// x of one lane, wave-uniform
__device__ __forceinline__ double readlane_f64(double x, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), lane), __builtin_amdgcn_readlane(__double2loint(x), lane));
}

// The span that ends at position n (optional spans, la_viterbi.hip): skip_row[n] = a with 0 <= a < n declares labels a .. n-1 optional.
// span_first: a, or -1 for none (position 0, or a outside 0 <= a < n); skip_row is not null.
__device__ __forceinline__ int span_first(const int32_t *skip_row, int n) {
    if (n < 1) return -1;
    const int a = skip_row[n];
    return a >= 0 && a < n ? a : -1;
}
// What the span gives state k at its position n = k >> 1: the jump sources J = 2a (the silence before the span) and, where jm1_ok, J-1
// (the label before it: a >= 1, and for an odd target only when labels[n] != labels[a-1]).  J = -1: none -- a null skip_row, a state
// past the clip's last, or no span at n.
struct SpanSource {
    int J;
    bool jm1_ok;
};
__device__ __forceinline__ SpanSource span_source(const int32_t *skip_row, const int32_t *lab, int k, bool valid) {
    SpanSource s{-1, false};
    const int n = k >> 1;
    const int a = skip_row && valid ? span_first(skip_row, n) : -1;
    if (a >= 0) {
        s.J = 2 * a;
        s.jm1_ok = a >= 1 && (!(k & 1) || lab[n] != lab[a - 1]);
    }
    return s;
}

// The repeat span that starts at label a (repeatable spans, la_viterbi.hip): repeat_row[a] = e with a < e <= L declares labels a .. e-1
// repeatable -- having finished label e-1 the path may return to label a.  What it gives state k: only the odd state 2a+1 is a target;
// its sources are K = 2e (the silence after the span) and, where km1_ok, K-1 (label e-1: only when labels[a] != labels[e-1], the
// equal-neighbour rule, so a one-label span returns through the silence alone).  K = -1: none -- a null repeat_row, an even state, a
// state past the clip's last, or any entry outside a < e <= L (never used as an index).
struct RepeatSource {
    int K;
    bool km1_ok;
};
__device__ __forceinline__ RepeatSource repeat_source(const int32_t *repeat_row, const int32_t *lab, int k, bool valid, int L) {
    RepeatSource s{-1, false};
    if (repeat_row && valid && (k & 1)) {
        const int a = k >> 1;
        const int e = repeat_row[a];
        if (e > a && e <= L) {
            s.K = 2 * e;
            s.km1_ok = lab[a] != lab[e - 1];
        }
    }
    return s;
}

// log(exp(a) + exp(b) [+ exp(c)]), -inf safe: float64 maximum, float32 correction.  The correction log(sum exp(x - max)) lies
// in [0, ln 3], so its float32 rounding is <= ~1e-7 absolute per step while the path scores themselves stay float64.
__device__ __forceinline__ double log_add3(double a, double b, double c) {
    const double m = fmax(a, fmax(b, c));
    if (m == -INFINITY) return -INFINITY;
    const float sum = __expf((float)(a - m)) + __expf((float)(b - m)) + __expf((float)(c - m));
    return m + (double)__logf(sum);
}
__device__ __forceinline__ double log_add2(double a, double b) {
    const double m = fmax(a, b);
    if (m == -INFINITY) return -INFINITY;
    const float sum = __expf((float)(a - m)) + __expf((float)(b - m));
    return m + (double)__logf(sum);
}
// log(exp(a) + exp(b)), -inf safe, all float64.  Path scores reach -T*log(V) ~ -1e4, where float32 has ~1e-3 absolute
// resolution and the occupancies exp(alpha+beta+nll-lp) lose 2-3 digits over a 1500-step recursion (measured 0.4 %).
__device__ __forceinline__ double log_add(double a, double b) {
    const double m = fmax(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + log1p(exp(fmin(a, b) - m));
}
// log_add with its trivial cases taken first -- the same values to the bit (log1p(exp(-inf)) = 0) -- so that a wave in which no lane
// has two finite operands (no jump arc at this call site) skips the float64 exp / log1p.  The jump terms of the posterior sweeps
// (la_posterior.hip)
__device__ __forceinline__ double log_add_jump(double a, double b) {
    if (b == -INFINITY) return a;
    if (a == -INFINITY) return b;
    return log_add(a, b);
}

}  // namespace lattice
}  // namespace la
