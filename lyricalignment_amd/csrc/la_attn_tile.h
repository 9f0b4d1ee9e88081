// la_attn_tile.h -- what the register-resident flash attention kernels share (la_attention.hip: the 16-bit inference kernel and, for the
// block order and the row store, the float32 one; la_attention_f16x2.hip: the f16x2 forward and its two backward sweeps): the block order,
// the swizzled 64-row LDS images with their LDS-DMA staging and their two fragment reads, the fragment pin, the two-buffer sweep and the
// row epilogue; on the host side the workspace carver and the argument checks of the forward entry points.
#pragma once
#include <type_traits>

#include "la_common.h"

namespace la {
namespace attn {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

constexpr int KT = 64;                  // keys per tile
constexpr int IMG = KT * 128;           // one image: [64 token rows][128 B = 64 sixteen-bit columns of one head]
constexpr float kLog2e = 1.4426950408889634f;

// Block -> (query tile, head, clip).  Workgroups are dealt round-robin over the 8 XCDs in launch order and every XCD has its
// own 4 MiB L2, so with the natural order the query tiles of one (clip, head) -- which all sweep the same 384 KiB of K and V
// -- land on 8 different L2s and the chip-wide in-flight K/V set (~40 MB) thrashes every one of them.  With (clip, head)
// pairs a multiple of 8, launch slot L goes to XCD L % 8 and that XCD's slots walk (pair, query tile) with the tile
// fastest: a pair's tiles share one L2 and ~13 pairs are in flight per XCD.  Otherwise the natural order is kept.
struct BlockCoord { int qt, head, clip; };
__device__ __forceinline__ BlockCoord block_coord(int nq, int n_head, int batch) {
    const int L = blockIdx.x, pairs = n_head * batch;
    int pair, qt;
    if ((pairs & 7) == 0) {
        const int x = L & 7, idx = L >> 3;
        pair = x + 8 * (idx / nq);
        qt = idx % nq;
    } else {
        pair = L / nq;
        qt = L % nq;
    }
    return BlockCoord{qt, pair % n_head, pair / n_head};
}

// accumulator register -> row (key / dv index) inside a 32x32 tile for lane half h
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// An image read by rows (ds_read_b128):               16-B slot s of row r stored at slot s ^ ((r >> 1) & 7)
// An image read transposed (ds_read_b64_tr_b16):      slot s of row r stored at slot s ^ (((r >> 1) & 1) << 2)
__device__ __forceinline__ int kswz(int r) { return (r >> 1) & 7; }
__device__ __forceinline__ int vswz(int r) { return ((r >> 1) & 1) << 2; }

// Staging: a piece = rows 8i .. 8i+7 of one image (16 B per lane); wave w brings pieces w * PER .. + PER - 1 (PER = 8 / waves per
// workgroup).  The per-lane byte offset of a piece (tile row * pitch + source-side swizzled slot; k = row-read image, v = transposed-read
// image) is loop invariant; the tile advance is a scalar base bump.  Rows past the end of the sequence (last tile only) are clamped to
// its last row -- they are masked to -inf in the scores.  A token row is `pitch` elements of ES bytes from the next: ES = 2 for 16-bit
// rows [token][ld], ES = 4 for the half planes [token][2][C] of a float32 operand (pitch = C).
template <int PER> struct KvOff { unsigned k[PER], v[PER]; };
template <int PER, int ES>
__device__ __forceinline__ KvOff<PER> kv_offsets(int64_t pitch, int key0, int T, int wave, int lane) {
    KvOff<PER> o;
    const int ps = lane & 7, r8 = lane >> 3;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int r = (wave * PER + i) * 8 + r8;
        const int rr = key0 + r < T ? r : T - 1 - key0;
        o.k[i] = (unsigned)(rr * pitch * ES) + ((ps ^ kswz(r)) << 4);
        o.v[i] = (unsigned)(rr * pitch * ES) + ((ps ^ vswz(r)) << 4);
    }
    return o;
}
// this wave's pieces of two images that travel together -- a K and a V tile (skip1 = 0), or the hi and the lo plane of one operand tile
// (src1 = src0, skip1 = the elements from a token's hi to its lo plane): src = the tile's first token row at the head's columns, buf = the
// image's LDS address.  POL (la_common.h CachePol, option cp_attn_kv): the cache policy in the text of the LDS-DMA pieces
template <int PER, int POL = 0>
__device__ __forceinline__ void stage_pair(const unsigned short *src0, const unsigned (&off0)[PER], unsigned buf0, const unsigned short *src1,
                                           int64_t skip1, const unsigned (&off1)[PER], unsigned buf1, int wave) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        la::glds16_so_pol<POL>(off0[i], src0, buf0 + (wave * PER + i) * 1024);
        la::glds16_so_pol<POL>(off1[i], src1 + skip1, buf1 + (wave * PER + i) * 1024);
    }
}

// Fragment readers.  Row fragment (M = token row of the image, K = 16 columns of the head dimension: c): ds_read_b128
template <typename V>
__device__ __forceinline__ V row_frag(const unsigned char *img, int row, int c, int h) {
    return __builtin_bit_cast(V, *reinterpret_cast<const uint4 *>(img + row * 128 + (((2 * c + h) ^ kswz(row)) << 4)));
}
// Transposed fragment (A operand, M = 32 columns of the head dimension: b, K = 16 token rows tok0 ..): lane (col = 32b + 16(g&1) + (lane&15),
// half g>>1) gets token rows tok0 + 4(g>>1) + {0..3} and + 8
// (g = lane >> 4, q4 = (lane & 15) >> 2, pp = lane & 3: three plain constants of the kernel)
template <typename V>
__device__ __forceinline__ V tr_frag(const unsigned char *img, int tok0, int b, int g, int q4, int pp) {
    const int key0 = tok0 + 4 * (g >> 1);
    const int slot = b * 4 + 2 * (g & 1) + (pp >> 1);
    const int r0 = key0 + q4, r1 = key0 + 8 + q4;
    typedef __attribute__((address_space(3))) s16x4 *lds_s16x4;
    const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(img + r0 * 128 + ((slot ^ vswz(r0)) << 4) + (pp & 1) * 8));
    const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(img + r1 * 128 + ((slot ^ vswz(r1)) << 4) + (pp & 1) * 8));
    return __builtin_bit_cast(V, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
}

// The fragments a wave loads once from global memory are "used" here, before the tile loop, so that hipcc places its own wait for their
// loads there.  Left to itself it waits at their first use inside the loop (vmcnt(3) .. vmcnt(0) ahead of the S MFMAs), and in steady
// state those counts no longer refer to the fragment loads but to the staging loads of the NEXT tile just issued: every tile then stalls
// on its successor's K / V arriving instead of letting them land under the softmax and PV phases.  (One statement for the fragments of
// one K-step: the waits come out per statement.)
template <typename... F>
__device__ __forceinline__ void pin_frags(uint4 &a, F &...more) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    static_assert(sizeof...(F) == 0 || sizeof...(F) == 1 || sizeof...(F) == 3, "one, two or four fragments");
    uint4 *f[] = {&a, &more...};
    u32x4 t[1 + sizeof...(F)];
#pragma unroll
    for (unsigned i = 0; i < 1 + sizeof...(F); ++i) t[i] = __builtin_bit_cast(u32x4, *f[i]);
    if constexpr (sizeof...(F) == 0) asm volatile("" : "+v"(t[0]));
    else if constexpr (sizeof...(F) == 1) asm volatile("" : "+v"(t[0]), "+v"(t[1]));
    else asm volatile("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]));
#pragma unroll
    for (unsigned i = 0; i < 1 + sizeof...(F); ++i) *f[i] = __builtin_bit_cast(uint4, t[i]);
}

// The sweep over tiles t0 .. n-1 with two LDS buffers: step(t, buffer) is instantiated once per buffer, so every fragment address is
// (loop-invariant VGPR) + immediate
template <typename Step>
__device__ __forceinline__ void sweep2(int t0, int n, Step &&step) {
    for (int t = t0; t < n; t += 2) {
        step(t, std::integral_constant<int, 0>{});
        if (t + 1 < n) step(t + 1, std::integral_constant<int, 1>{});
    }
}

// Epilogue of an O^T / dQ^T / dK^T / dV^T accumulator pair: lane (row, half h) holds columns 32 b + 8 r4 + 4 h .. + 3 of its row in
// registers 4 r4 .. + 3 of acc[b]
__device__ __forceinline__ void store_row_scaled(float *row, const f32x16 (&acc)[2], float scale, int h) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
            *reinterpret_cast<float4 *>(row + 32 * b + 8 * r4 + 4 * h) =
                make_float4(acc[b][4 * r4 + 0] * scale, acc[b][4 * r4 + 1] * scale, acc[b][4 * r4 + 2] * scale, acc[b][4 * r4 + 3] * scale);
}

// ---- host side ----
// Workspace carver: consecutive 256-byte aligned pieces of one allocation (base may be null: only `off`, the size, is wanted)
struct Carver {
    char *base;
    size_t off = 0;
    template <typename T> T *take(size_t count) {
        T *p = reinterpret_cast<T *>(base + off);
        off += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

// The argument checks the forward entry points share, in their order: pointers and sizes (ptrs_ok: the entry's own pointers are all there),
// the element type with its LA_Q_LOG2 rider, the entry's own condition (own_error: its message, or null), leading dimensions (q rows hold
// at least q_cols values), 16-byte alignment of every row.  Messages are "<entry>: <what>".
inline int check_forward_args(const char *entry, int dtype_arg, bool ptrs_ok, const void *q, const void *k, const void *v, const void *out,
                              int64_t ld_q, int64_t q_cols, int64_t ld_kv, int64_t ld_out, int batch, int q_len, int kv_len, int n_head,
                              const char *own_error) {
    LA_CHECK_ARG(ptrs_ok && batch > 0 && q_len > 0 && kv_len > 0 && n_head > 0, "%s: bad arguments", entry);
    const int dtype = dtype_arg & 0xff;       // LA_Q_LOG2 may ride on it
    LA_CHECK_ARG((dtype_arg & ~(0xff | LA_Q_LOG2)) == 0 && (dtype == LA_F32 || dtype == LA_BF16 || dtype == LA_F16), "%s: bad dtype", entry);
    LA_CHECK_ARG(!own_error, "%s: %s", entry, own_error);
    const int es = dtype == LA_F32 ? 4 : 2;
    LA_CHECK_ARG(ld_q >= q_cols && ld_kv >= n_head * 64 && ld_out >= n_head * 64, "%s: leading dimensions too small", entry);
    LA_CHECK_ARG((ld_q * es) % 16 == 0 && (ld_kv * es) % 16 == 0 && (ld_out * es) % 16 == 0 && (uintptr_t)q % 16 == 0 &&
                     (uintptr_t)k % 16 == 0 && (uintptr_t)v % 16 == 0 && (uintptr_t)out % 16 == 0,
                 "%s: rows must be 16-byte aligned", entry);
    return LA_OK;
}

}  // namespace attn
}  // namespace la
