// la_row.h -- the ONE definition of what the row kernels share (device helpers only):
//   * the whole-wave float butterflies and the pairwise combine of a 256-thread workgroup's four waves.  A row normaliser's bits are its
//     reduction order: kernels that promise each other's bits (la_emissions_from_logits / la_anchored_alignment_loss, DESIGN.md
//     "Alignment loss on the windowed lattice") keep the promise by calling these, not by parallel text;
//   * the emission formulas of the reference (utils/alignment.py:123-134, :14-20), shared by the fused head's merge (la_head.hip), the
//     prep from materialised logits (la_elementwise.hip) and the anchored loss (la_anchor_loss.hip).  Each kernel keeps its own
//     class-range test.
// Butterflies over doubles, (value, index) pairs, integers and parts of a wave stay with their kernels.
#pragma once
#include "la_common.h"

namespace la {

// xor butterflies 32 -> 1: every lane ends with the wave's result
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// 256-thread workgroup: butterfly, one LDS slot per wave, ONE barrier, the four waves combined pairwise.  The caller owns the four slots:
// a second reduction on other slots (red / red + 4) needs no barrier between the first one's reads and its own stores.
__device__ __forceinline__ float block4_max(float v, float *red4) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red4[0], red4[1]), fmaxf(red4[2], red4[3]));
}
__device__ __forceinline__ float block4_sum(float v, float *red4) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red4[0] + red4[1]) + (red4[2] + red4[3]);
}

// ---- emissions: x a logit of the row, m / logsum the row's maximum and log sum exp(x - m) over the normaliser's columns, kept apart ----
constexpr float kEmissionFloor = -1000.0f;   // the reference's clamp (:134, :20); also the emission of a class id outside the range

// CTC variant: log sigmoid(xs) and log(1 - sigmoid(xs)) of the silence logit, in the reference's naive forms ON PURPOSE (:125-129):
// log_voiced may be -inf where log1p(-sil) would not be
struct SilenceTerms {
    float log_sil, log_voiced;
};
__device__ __forceinline__ SilenceTerms silence_terms(float xs) {
    const float sil = sigmoidf_(xs);                       // F.sigmoid (:125)
    return SilenceTerms{logf(sil), logf(1.0f - sil)};      // (:128), (:126,:129)
}
__device__ __forceinline__ float silence_emission(float log_sil) { return fmaxf(log_sil, kEmissionFloor); }   // (:134)
__device__ __forceinline__ float voiced_emission(float x, float m, float logsum, float log_voiced) {           // (:131-132)
    return fmaxf(((x - m) - logsum) + log_voiced, kEmissionFloor);
}
__device__ __forceinline__ float plain_emission(float x, float m, float logsum) {                              // (:16-20)
    return fmaxf((x - m) - logsum, kEmissionFloor);
}

}  // namespace la
