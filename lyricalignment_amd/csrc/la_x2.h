// la_x2.h -- the split arithmetic of the "f16x2" scheme, stated once for every kernel that splits (la_f32x2.hip, la_attention_f16x2.hip,
// la_gru.hip): a float32 value scaled by a power of two splits exactly into two IEEE halves hi + lo (22 bits), and a float32 product
// becomes three f16 MFMA products lo.hi + hi.lo + hi.hi accumulated in float32.
#pragma once
#include "la_common.h"

namespace la {
namespace x2 {

// power of two s with mx * s in [2^13, 2^14); mx == 0 (or not finite) -> 1.  Returns s, *inv = 1 / s (both exact).
// LIMIT bounds the shift: 126 keeps s and 1 / s normal; the GRU kernels pass 100, which also keeps their inv * 2^-14 normal.
template <int LIMIT = 126>
__device__ __forceinline__ float scale_for(float mx, float *inv) {
    if (!(mx > 0.f) || !(mx < 3.0e38f)) { *inv = 1.f; return 1.f; }
    int e;
    (void)frexpf(mx, &e);                    // mx = m 2^e, m in [0.5, 1)
    int sh = 14 - e;
    sh = sh > LIMIT ? LIMIT : (sh < -LIMIT ? -LIMIT : sh);
    *inv = ldexpf(1.f, -sh);
    return ldexpf(1.f, sh);
}

// xs (already scaled) -> hi = f16(xs), lo = f16(xs - hi), as bit patterns
__device__ __forceinline__ void split(float xs, unsigned short &hi, unsigned short &lo) {
    const _Float16 h = (_Float16)xs;
    const _Float16 l = (_Float16)(xs - (float)h);
    hi = __builtin_bit_cast(unsigned short, h);
    lo = __builtin_bit_cast(unsigned short, l);
}

// the same as one word: f16 hi | f16 lo << 16
__device__ __forceinline__ unsigned pack_hi_lo(float xs) {
    const _Float16 h = (_Float16)xs;
    const _Float16 l = (_Float16)(xs - (float)h);
    return (unsigned)__builtin_bit_cast(unsigned short, h) | ((unsigned)__builtin_bit_cast(unsigned short, l) << 16);
}

// two packed neighbours p0, p1 (pack_hi_lo of elements k, k + 1) -> the word of plane PLANE (0 = hi, 1 = lo) that holds them
template <int PLANE>
__device__ __forceinline__ unsigned plane_word(unsigned p0, unsigned p1) {
    return PLANE == 0 ? (p0 & 0xffffu) | (p1 << 16) : (p0 >> 16) | (p1 & 0xffff0000u);
}

// eight packed neighbours -> their 16 bytes of plane PLANE (one MFMA fragment)
template <int PLANE>
__device__ __forceinline__ uint4 plane_frag(const unsigned (&p)[8]) {
    return make_uint4(plane_word<PLANE>(p[0], p[1]), plane_word<PLANE>(p[2], p[3]), plane_word<PLANE>(p[4], p[5]), plane_word<PLANE>(p[6], p[7]));
}

}  // namespace x2
}  // namespace la
