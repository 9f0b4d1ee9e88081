// la_lattice.h -- what the kernels that sweep the alignment lattice (S = 2L+1 states, one lane per state, row by row) have in
// common: la_viterbi.hip (max-product), la_posterior.hip and the CTC lattice of la_loss.hip (sum-product).  Device helpers for
// the neighbour exchange inside one wave64 and for the log-sum-exp of a step, and the host's wave count of a label count.
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

}  // namespace lattice
}  // namespace la
