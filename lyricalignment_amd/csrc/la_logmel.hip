// la_logmel.hip -- log-mel front end on the device (replaces whisper.audio.log_mel_spectrogram,
// which the reference runs on the CPU and then copies over: module/align_model.py:84).
//
//   audio [B][N] --reflect pad 200--> frames (overlapping 400-sample rows, hop 160)
//     --windowed DFT [cos | sin] as an exact-f32 MFMA product--> re, im  --|.|^2--> power [201]
//     --Slaney mel filter bank [n_mels][201], exact-f32 MFMA--> mel
//     --log10(max(., 1e-10)), max over the WHOLE batch tensor, floor at max-8, (x+4)/4-->  [B][n_mels][N/160]
// n_mels = 80 (whisper tiny .. large-v2) or 128 (large-v3, large-v3-turbo): a template parameter of the tile and constants kernels.
// frame count = N / 160 (torch.stft(center=True) yields 1 + N/160 frames; upstream drops the last).
//
// Round 4: ONE kernel per 64-frame tile does everything up to the log (logmel_tile_kernel):
//   * the tile's 10480 waveform samples (64 hops + the 240-sample overlap, reflect padding resolved on the way in) are
//     staged once in LDS; the 64 x 400 frame matrix is the overlapping row view of that span (row pitch 160 floats),
//     never materialised;
//   * a wave owns 16 frames and all 2 x 208 DFT columns: 26 accumulator tiles of v_mfma_f32_16x16x4_f32 (k-ordered fmaf
//     chains = the parity mode's arithmetic), the DFT matrix streams from L2 in fragment order (256 B per wave load);
//   * re^2 + im^2 in the accumulator registers, through LDS once (16 x 208 per wave) to become the K operand of the mel
//     product (n_mels / 16 = 5 or 8 accumulator tiles), log10 and the tile's maximum in registers, the tile leaves through LDS
//     as whole 256-byte row segments of the [n_mels][frames] output.
// LDS: 80 bins keep the out tile [80][68] BEHIND the span / power tile (75,280 bytes, two workgroups per CU).  At 128 bins that
// arrangement would be 88,336 bytes and one workgroup per CU; the power tile is dead after the mel product, so there the out tile
// [128][68] takes ITS place behind one more barrier (53,520 bytes, still two workgroups per CU).
// Neither the spectrum [rows][416] nor the power [rows][224] of the first version exists in memory: HBM traffic is the
// waveform in (61 MB per 32 x 30 s), the log-mel out (31 MB) and one in-place pass for the whole-tensor floor
// (logmel_finish_kernel, 31 + 31 MB) = 1.7 x the 92 MB a log-mel must move; 2 launches (3 when the constants are built in
// the same call).  The constants (windowed DFT matrix in fragment order, padded filter bank) are built ONCE per
// (window, filters) pair by la_logmel_constants into a caller-owned buffer.
#include <algorithm>
#include <math.h>
#include <mutex>
#include <unordered_map>

#include "la_row.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int NFFT = 400, HOP = 160, NBIN = 201;
constexpr int FT = 64;                         // frames per workgroup tile (4 waves x 16)
constexpr int NCB = 13;                        // 16-bin column blocks per part: 208 >= 201 bins
constexpr int NBP = NCB * 16;                  // 208: padded bin count = K of the mel product (multiple of 4)
constexpr int SPAN = (FT - 1) * HOP + NFFT;    // 10480 samples feed one tile
constexpr int PWP = 209;                       // power row pitch in floats (odd: 16 rows x 4 k land on distinct banks)
constexpr int OUTP = 68;                       // out tile row pitch
constexpr int DFT_FLOATS = 2 * NCB * NFFT * 16;    // [26 column blocks][400 taps][16 columns]
constexpr int LDS_MAIN = FT * PWP > SPAN ? FT * PWP : SPAN;   // the power tile reuses the waveform span
constexpr int LDS_TWO_PER_CU = 80 * 1024;      // dynamic LDS with which two workgroups still share a CU (__launch_bounds__(256, 2))

// What the mel bin count decides: NMEL = 80 or 128.
template <int NMEL>
struct Bins {
    static_assert(NMEL % 16 == 0, "whole 16-row accumulator tiles");
    static constexpr int NMB = NMEL / 16;                       // 5 or 8 blocks of 16 mel rows
    static constexpr int FILT_FLOATS = NMB * NBP * 16;          // [NMB mel blocks][208 bins][16 mel rows]
    static constexpr int CONST_FLOATS = DFT_FLOATS + FILT_FLOATS;
    // the out tile [NMEL][OUTP] behind the span / power tile where that leaves room for two workgroups per CU (80 bins), else in the
    // power tile's place once the mel product has read it (128 bins)
    static constexpr bool OUT_OVER_POWER = (LDS_MAIN + NMEL * OUTP + 4) * 4 > LDS_TWO_PER_CU;
    static constexpr int OUT_AT = OUT_OVER_POWER ? 0 : LDS_MAIN;
    static constexpr int RED_AT = OUT_OVER_POWER ? LDS_MAIN : LDS_MAIN + NMEL * OUTP;
    static constexpr int LDS_FLOATS = RED_AT + 4;
    static_assert(!OUT_OVER_POWER || NMEL * OUTP <= LDS_MAIN, "the out tile must fit in the power tile's place");
    static_assert(LDS_FLOATS * 4 <= LDS_TWO_PER_CU, "two workgroups per CU");
};

// consts[0 .. DFT_FLOATS): Wt[cb][k][c] = window[k] * cos | sin (2 pi bin k / 400), bin = (cb % 13) * 16 + c, cb < 13: cos,
//   zero for bin >= 201 -- so the B fragment of (column block cb, k-step s) is the 64 consecutive floats at (cb * 400 + 4 s) * 16;
// consts[DFT_FLOATS ..): Fp[mb][bin][r] = filters[mb * 16 + r][bin], zero for bin >= 201: the A fragment of (mel block, k-step).
template <int NMEL>
__global__ void logmel_constants_kernel(const float *window, const float *filters, float *consts) {
    constexpr int FILT_FLOATS = Bins<NMEL>::FILT_FLOATS;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < DFT_FLOATS) {
        const int cb = idx / (NFFT * 16), k = (idx / 16) % NFFT, c = idx % 16;
        const int bin = (cb % NCB) * 16 + c;
        float v = 0.f;
        if (bin < NBIN) {
            const int ph = (int)(((long long)bin * k) % NFFT);   // exact phase reduction
            const double a = 2.0 * (double)ph / (double)NFFT;    // in units of pi
            v = (float)((double)window[k] * (cb < NCB ? cospi(a) : sinpi(a)));
        }
        consts[idx] = v;
    } else if (idx < DFT_FLOATS + FILT_FLOATS) {
        const int j = idx - DFT_FLOATS;
        const int mb = j / (NBP * 16), bin = (j / 16) % NBP, r = j % 16;
        consts[idx] = bin < NBIN ? filters[(mb * 16 + r) * NBIN + bin] : 0.f;
    }
}

// One 64-frame tile of one clip: waveform span -> log10 mel [NMEL][64] (unfloored) into mel[b][m][j0 ..], the maximum of the
// tile's valid values into blockmax[b * gridDim.x + tile].
// RAGGED (la_logmel_ragged_f32_prepared): the rows of `audio` are `row_len` samples apart and clip b owns the first n_samples[b] of its
// row: the reflect padding turns at the clip's own end, its frame count is n_samples[b] / 160, and a tile wholly past that does no DFT
// (its blockmax slot gets -inf; logmel_finish_ragged_kernel writes the zeros there).
template <int NMEL, bool RAGGED>
__global__ __launch_bounds__(256, 2) void logmel_tile_kernel(const float *__restrict__ audio, int row_len, int frames,
                                                             const float *__restrict__ consts, float *__restrict__ mel,
                                                             int64_t mbs, int64_t mrs, float *__restrict__ blockmax,
                                                             const int *__restrict__ n_samples) {
    constexpr int NMB = Bins<NMEL>::NMB;
    extern __shared__ float lds[];
    float *span = lds;                         // [SPAN] waveform, later pw[64][PWP]
    float *outt = lds + Bins<NMEL>::OUT_AT;    // [NMEL][OUTP]
    float *red = lds + Bins<NMEL>::RED_AT;     // [4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int b = blockIdx.y, j0 = blockIdx.x * FT;
    const float *a = audio + (int64_t)b * row_len;
    int N = row_len;
    if constexpr (RAGGED) {
        N = min(max(n_samples[b], 0), row_len);          // never past the row, whatever the caller's array holds
        frames = N / HOP;
        if (j0 >= frames) {                              // (uniform over the workgroup: before the first barrier)
            if (tid == 0) blockmax[(int64_t)b * gridDim.x + blockIdx.x] = -INFINITY;
            return;
        }
    }

    // ---- the tile's span of the reflect-padded waveform: padded[p] = audio[reflect(p - 200)], zero past N + 400 ----
    const int64_t p0 = (int64_t)j0 * HOP;
    for (int i = tid; i < SPAN; i += 256) {
        const int64_t p = p0 + i;
        float v = 0.f;
        if (p < (int64_t)N + NFFT) {
            int64_t s = p - NFFT / 2;
            if (s < 0) s = -s;
            if (s >= N) s = 2 * (int64_t)(N - 1) - s;
            s = s < 0 ? 0 : s;   // only for N < 201, where torch.stft itself refuses the reflect pad
            v = a[s];
        }
        span[i] = v;
    }
    __syncthreads();

    // ---- DFT: [16 frames of this wave] x [400 taps] x [26 column blocks] ----
    f32x4 acc[2 * NCB];
#pragma unroll
    for (int c = 0; c < 2 * NCB; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float *xa = span + (16 * wave + lr) * HOP + lq;       // A: frame lr of the wave, tap 4 s + lq
    const float *wt = consts + lane;                            // B: (cb * 400 + 4 s) * 16 + lane
    float bcur[2 * NCB], bnext[2 * NCB];
#pragma unroll
    for (int c = 0; c < 2 * NCB; ++c) bcur[c] = wt[(int64_t)c * NFFT * 16];
    for (int s = 0; s < NFFT / 4; ++s) {
        const int sn = s + 1 < NFFT / 4 ? s + 1 : s;
#pragma unroll
        for (int c = 0; c < 2 * NCB; ++c) bnext[c] = wt[((int64_t)c * NFFT + 4 * sn) * 16];
        const float av = xa[4 * s];
#pragma unroll
        for (int c = 0; c < 2 * NCB; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bcur[c], acc[c], 0, 0, 0);
#pragma unroll
        for (int c = 0; c < 2 * NCB; ++c) bcur[c] = bnext[c];
    }
    __syncthreads();   // every wave is done with the waveform span: the power tile takes its place

    // ---- power = re^2 + im^2: lane holds bins cb * 16 + lr of frames 4 lq + r; rows of this wave only ----
    float *pw = span + (16 * wave) * PWP;
#pragma unroll
    for (int c = 0; c < NCB; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) pw[(4 * lq + r) * PWP + c * 16 + lr] = acc[c][r] * acc[c][r] + acc[NCB + c][r] * acc[NCB + c][r];
    __syncthreads();

    // ---- mel^T[NMEL][16 frames] = filters [NMEL][208] x power^T [208][16 frames] ----
    f32x4 macc[NMB];
#pragma unroll
    for (int m = 0; m < NMB; ++m) macc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float *fp = consts + DFT_FLOATS + lane;               // A: (mb * 208 + 4 s) * 16 + lane
    const float *pb = pw + lr * PWP + lq;                       // B: power[frame lr][bin 4 s + lq]
#pragma unroll 4
    for (int s = 0; s < NBP / 4; ++s) {
        const float bv = pb[4 * s];
#pragma unroll
        for (int m = 0; m < NMB; ++m) macc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(fp[(m * NBP + 4 * s) * 16], bv, macc[m], 0, 0, 0);
    }
    if constexpr (Bins<NMEL>::OUT_OVER_POWER) __syncthreads();   // every wave is done with the power tile: the out tile takes its place

    // ---- log10, the tile's maximum over real frames, tile out through LDS as whole row segments ----
    const bool live = j0 + 16 * wave + lr < frames;
    float mx = -INFINITY;
#pragma unroll
    for (int m = 0; m < NMB; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = log10f(fmaxf(macc[m][r], 1e-10f));
            if (live) mx = fmaxf(mx, v);
            outt[(m * 16 + 4 * lq + r) * OUTP + 16 * wave + lr] = v;
        }
    mx = la::block4_max(mx, red);
    if (tid == 0) blockmax[(int64_t)b * gridDim.x + blockIdx.x] = mx;
    const int f = tid & 63;
    if (j0 + f < frames) {
        float *dst = mel + (int64_t)b * mbs + j0 + f;
        for (int m = tid >> 6; m < NMEL; m += 4) dst[(int64_t)m * mrs] = outt[m * OUTP + f];
    }
}

// mel[b][m][j] <- (max(v, gmax - 8) + 4) / 4 in place, gmax = the maximum over every tile of the call.
// One workgroup per (4 mel rows, clip).
__global__ __launch_bounds__(256) void logmel_finish_kernel(float *mel, int64_t mbs, int64_t mrs, int frames,
                                                            const float *blockmax, int nblockmax) {
    __shared__ float red[4];
    float m = -INFINITY;
    for (int i = threadIdx.x; i < nblockmax; i += 256) m = fmaxf(m, blockmax[i]);
    const float floor_v = la::block4_max(m, red) - 8.0f;
    for (int r = 0; r < 4; ++r) {
        float *row = mel + (int64_t)blockIdx.y * mbs + (int64_t)(blockIdx.x * 4 + r) * mrs;
        for (int j = threadIdx.x; j < frames; j += 256) row[j] = (fmaxf(row[j], floor_v) + 4.0f) / 4.0f;
    }
}

// The ragged form's finish: clip b's floor from the maximum over ITS tiles, frames j < n_samples[b] / 160 floored and scaled in place,
// literal zeros from there to out_frames (whisper's pad_or_trim of the clip's own log-mel).  One workgroup per (4 mel rows, clip).
__global__ __launch_bounds__(256) void logmel_finish_ragged_kernel(float *mel, int64_t mbs, int64_t mrs, int out_frames, const int *n_samples,
                                                                   int row_len, const float *blockmax, int tiles) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < tiles; i += 256) m = fmaxf(m, blockmax[(int64_t)b * tiles + i]);
    const float floor_v = la::block4_max(m, red) - 8.0f;
    const int frames = min(min(max(n_samples[b], 0), row_len) / HOP, out_frames);
    for (int r = 0; r < 4; ++r) {
        float *row = mel + (int64_t)b * mbs + (int64_t)(blockIdx.x * 4 + r) * mrs;
        for (int j = threadIdx.x; j < out_frames; j += 256) row[j] = j < frames ? (fmaxf(row[j], floor_v) + 4.0f) / 4.0f : 0.f;
    }
}

bool bins_ok(int n_mels) { return n_mels == 80 || n_mels == 128; }
#define LA_CHECK_BINS(n_mels, what) LA_CHECK_ARG(bins_ok(n_mels), what ": n_mels = %d, the kernels are built for 80 or 128", (int)(n_mels))

size_t const_bytes(int n_mels) { return (size_t)(n_mels == 128 ? Bins<128>::CONST_FLOATS : Bins<80>::CONST_FLOATS) * 4; }

// Which bin count a constants buffer was filled for, by its address (include/lyricalign.h states the rule): written by
// la_logmel_constants(_n) after its launch, read by the prepared entries before theirs.  0 = no record.
std::mutex consts_mutex;
std::unordered_map<const void *, int> consts_bins;

void note_constants(const void *consts, int n_mels) {
    std::lock_guard<std::mutex> g(consts_mutex);
    consts_bins[consts] = n_mels;
}

int check_constants(const void *consts, int n_mels, const char *what) {
    int have = 0;
    {
        std::lock_guard<std::mutex> g(consts_mutex);
        auto it = consts_bins.find(consts);
        if (it != consts_bins.end()) have = it->second;
    }
    // a buffer without a record can only be an 80-bin one (filled through another copy of this library, or a copy of such a buffer):
    // la_logmel_f32_prepared has always taken those
    LA_CHECK_ARG(have == n_mels || (have == 0 && n_mels == 80),
                 "%s: these constants were %s, this call is for %d (build them with la_logmel_constants_n(%d, ...) into this buffer)", what,
                 have == 80 ? "built for 80 mel bins" : have == 128 ? "built for 128 mel bins" : "not built by la_logmel_constants_n at this address",
                 n_mels, n_mels);
    return LA_OK;
}

struct MelPlan {
    int frames, tiles;
    size_t off_consts, off_bmax, total;
};

MelPlan plan_mel(int n_mels, int batch, int n_samples) {
    MelPlan p;
    p.frames = n_samples / HOP;
    p.tiles = la::cdiv(p.frames, FT);
    size_t o = 0;
    auto take = [&](int64_t bytes) { size_t r = o; o += (size_t)la::round_up(bytes, 256); return r; };
    p.off_consts = take((int64_t)const_bytes(n_mels));
    p.off_bmax = take((int64_t)batch * p.tiles * 4);
    p.total = o;
    return p;
}

template <int NMEL>
int launch_constants(const float *mel_filters, const float *window, void *consts, hipStream_t stream) {
    hipLaunchKernelGGL(logmel_constants_kernel<NMEL>, dim3(la::cdiv(Bins<NMEL>::CONST_FLOATS, 256)), dim3(256), 0, stream, window, mel_filters,
                       reinterpret_cast<float *>(consts));
    LA_LAUNCH_CHECK();
    return LA_OK;
}

int build_constants(int n_mels, const float *mel_filters, const float *window, void *consts, hipStream_t stream) {
    return n_mels == 128 ? launch_constants<128>(mel_filters, window, consts, stream) : launch_constants<80>(mel_filters, window, consts, stream);
}

// The tile kernel and its finish: the dense form (n_clip null: every clip has `row_len` samples, one floor for the whole call, `frames`
// frames written) or the ragged one (n_clip [batch] on the device: per-clip floor, zeros from the clip's end to `out_frames`).
template <int NMEL, bool RAGGED>
int launch_tiles(const float *audio, int batch, int row_len, const int *n_clip, const float *consts, float *mel, int64_t mbs, int64_t mrs,
                 int out_frames, float *bmax, const MelPlan &p, hipStream_t stream) {
    constexpr int LDS_BYTES = Bins<NMEL>::LDS_FLOATS * 4;
    static la::DeviceOnce attr_once;
    if (attr_once.pending()) {
        LA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(logmel_tile_kernel<NMEL, RAGGED>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   LDS_BYTES));
        attr_once.mark();
    }
    hipLaunchKernelGGL((logmel_tile_kernel<NMEL, RAGGED>), dim3(p.tiles, batch), dim3(256), LDS_BYTES, stream, audio, row_len, p.frames, consts,
                       mel, mbs, mrs, bmax, n_clip);
    if constexpr (RAGGED)
        hipLaunchKernelGGL(logmel_finish_ragged_kernel, dim3(NMEL / 4, batch), dim3(256), 0, stream, mel, mbs, mrs, out_frames, n_clip, row_len,
                           bmax, p.tiles);
    else
        hipLaunchKernelGGL(logmel_finish_kernel, dim3(NMEL / 4, batch), dim3(256), 0, stream, mel, mbs, mrs, p.frames, bmax, batch * p.tiles);
    LA_LAUNCH_CHECK();
    return LA_OK;
}

int run_logmel(int n_mels, const float *audio, int batch, int n_samples, const float *consts, float *mel, int64_t mbs, int64_t mrs,
               float *bmax, const MelPlan &p, hipStream_t stream) {
    return n_mels == 128 ? launch_tiles<128, false>(audio, batch, n_samples, nullptr, consts, mel, mbs, mrs, p.frames, bmax, p, stream)
                         : launch_tiles<80, false>(audio, batch, n_samples, nullptr, consts, mel, mbs, mrs, p.frames, bmax, p, stream);
}

int logmel_checks(const float *audio, int32_t batch, int32_t n_samples, float *mel, int64_t mel_row_stride, void *workspace,
                  size_t workspace_bytes, const MelPlan &p) {
    LA_CHECK_ARG(audio && mel && workspace, "logmel: null pointer");
    LA_CHECK_ARG(batch > 0 && n_samples > NFFT / 2, "logmel: need more than %d samples (reflect padding)", NFFT / 2);
    LA_CHECK_ARG(batch <= 65535, "logmel: at most 65535 clips per call");
    LA_CHECK_ARG((uintptr_t)workspace % 256 == 0, "logmel: workspace must be 256-byte aligned");
    LA_CHECK_ARG(p.frames >= 1 && mel_row_stride >= p.frames, "logmel: mel_row_stride < n_frames");
    LA_CHECK_ARG(workspace_bytes >= p.total, "logmel: workspace too small (%zu < %zu)", workspace_bytes, p.total);
    return LA_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// The entries that take the bin count; the 80-bin names below them are their n_mels = 80 calls.
extern "C" int la_logmel_constants_bytes_n(int32_t n_mels, size_t *bytes) {
    LA_CHECK_ARG(bytes, "logmel_constants_bytes: null pointer");
    LA_CHECK_BINS(n_mels, "logmel_constants_bytes");
    *bytes = const_bytes(n_mels);
    return LA_OK;
}

extern "C" int la_logmel_constants_n(int32_t n_mels, const float *mel_filters, const float *window, void *consts, size_t consts_bytes,
                                     void *stream_) {
    LA_CHECK_BINS(n_mels, "logmel_constants");
    LA_CHECK_ARG(mel_filters && window && consts, "logmel_constants: null pointer");
    LA_CHECK_ARG(consts_bytes >= const_bytes(n_mels) && (uintptr_t)consts % 16 == 0, "logmel_constants: buffer too small or not 16-byte aligned");
    int rc = build_constants(n_mels, mel_filters, window, consts, (hipStream_t)stream_);
    if (rc == LA_OK) note_constants(consts, n_mels);
    return rc;
}

extern "C" int la_logmel_workspace_bytes_n(int32_t n_mels, int32_t batch, int32_t n_samples, size_t *bytes) {
    LA_CHECK_ARG(bytes && batch > 0 && n_samples >= HOP, "logmel_workspace_bytes: bad arguments");
    LA_CHECK_BINS(n_mels, "logmel_workspace_bytes");
    *bytes = plan_mel(n_mels, batch, n_samples).total;
    return LA_OK;
}

// constants built inside the call (3 launches)
extern "C" int la_logmel_f32_n(int32_t n_mels, const float *audio, int32_t batch, int32_t n_samples, const float *mel_filters,
                               const float *window, float *mel, int64_t mel_batch_stride, int64_t mel_row_stride, void *workspace,
                               size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    LA_CHECK_BINS(n_mels, "logmel");
    LA_CHECK_ARG(mel_filters && window, "logmel: null pointer");
    const MelPlan p = plan_mel(n_mels, batch > 0 ? batch : 1, n_samples >= HOP ? n_samples : HOP);
    int rc = logmel_checks(audio, batch, n_samples, mel, mel_row_stride, workspace, workspace_bytes, p);
    if (rc != LA_OK) return rc;
    unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
    la::TimerScope ts("logmel", stream);
    rc = build_constants(n_mels, mel_filters, window, ws + p.off_consts, stream);      // (the workspace's own: no record kept of them)
    if (rc != LA_OK) return rc;
    return run_logmel(n_mels, audio, batch, n_samples, reinterpret_cast<const float *>(ws + p.off_consts), mel, mel_batch_stride,
                      mel_row_stride, reinterpret_cast<float *>(ws + p.off_bmax), p, stream);
}

// constants from la_logmel_constants_n (2 launches)
extern "C" int la_logmel_f32_prepared_n(int32_t n_mels, const float *audio, int32_t batch, int32_t n_samples, const void *consts, float *mel,
                                        int64_t mel_batch_stride, int64_t mel_row_stride, void *workspace, size_t workspace_bytes,
                                        void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    LA_CHECK_BINS(n_mels, "logmel");
    LA_CHECK_ARG(consts && (uintptr_t)consts % 16 == 0, "logmel: constants missing or misaligned");
    const MelPlan p = plan_mel(n_mels, batch > 0 ? batch : 1, n_samples >= HOP ? n_samples : HOP);
    int rc = logmel_checks(audio, batch, n_samples, mel, mel_row_stride, workspace, workspace_bytes, p);
    if (rc != LA_OK) return rc;
    rc = check_constants(consts, n_mels, "logmel");
    if (rc != LA_OK) return rc;
    unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
    la::TimerScope ts("logmel", stream);
    return run_logmel(n_mels, audio, batch, n_samples, reinterpret_cast<const float *>(consts), mel, mel_batch_stride, mel_row_stride,
                      reinterpret_cast<float *>(ws + p.off_bmax), p, stream);
}

// Ragged form: clip b = the first n_samples[b] (device) samples of row b of audio [batch][max_samples]; mel [batch][n_mels][out_frames]
// receives the clip's OWN log-mel (reflect padding at its own end, floor at its own maximum - 8) in frames 0 .. n_samples[b] / 160 - 1 and
// zeros from there to out_frames.  Two launches, the workspace of la_logmel_workspace_bytes_n(n_mels, batch, max_samples).
extern "C" int la_logmel_ragged_f32_prepared_n(int32_t n_mels, const float *audio, const int32_t *n_samples, int32_t batch, int32_t max_samples,
                                               const void *consts, float *mel, int64_t mel_batch_stride, int64_t mel_row_stride,
                                               int32_t out_frames, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    LA_CHECK_BINS(n_mels, "logmel_ragged");
    LA_CHECK_ARG(consts && (uintptr_t)consts % 16 == 0, "logmel_ragged: constants missing or misaligned");
    LA_CHECK_ARG(n_samples, "logmel_ragged: n_samples missing");
    const MelPlan p = plan_mel(n_mels, batch > 0 ? batch : 1, max_samples >= HOP ? max_samples : HOP);
    int rc = logmel_checks(audio, batch, max_samples, mel, mel_row_stride, workspace, workspace_bytes, p);
    if (rc != LA_OK) return rc;
    LA_CHECK_ARG(out_frames >= p.frames && mel_row_stride >= out_frames, "logmel_ragged: out_frames < max_samples / 160 or mel_row_stride < out_frames");
    rc = check_constants(consts, n_mels, "logmel_ragged");
    if (rc != LA_OK) return rc;
    float *bmax = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(workspace) + p.off_bmax);
    const float *c = reinterpret_cast<const float *>(consts);
    la::TimerScope ts("logmel", stream);
    return n_mels == 128
               ? launch_tiles<128, true>(audio, batch, max_samples, n_samples, c, mel, mel_batch_stride, mel_row_stride, out_frames, bmax, p, stream)
               : launch_tiles<80, true>(audio, batch, max_samples, n_samples, c, mel, mel_batch_stride, mel_row_stride, out_frames, bmax, p, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// The 80-bin names.
extern "C" int la_logmel_constants_bytes(size_t *bytes) { return la_logmel_constants_bytes_n(80, bytes); }

extern "C" int la_logmel_constants(const float *mel_filters, const float *window, void *consts, size_t consts_bytes, void *stream) {
    return la_logmel_constants_n(80, mel_filters, window, consts, consts_bytes, stream);
}

extern "C" int la_logmel_workspace_bytes(int32_t batch, int32_t n_samples, size_t *bytes) {
    return la_logmel_workspace_bytes_n(80, batch, n_samples, bytes);
}

extern "C" int la_logmel_f32(const float *audio, int32_t batch, int32_t n_samples, const float *mel_filters, const float *window, float *mel,
                             int64_t mel_batch_stride, int64_t mel_row_stride, void *workspace, size_t workspace_bytes, void *stream) {
    return la_logmel_f32_n(80, audio, batch, n_samples, mel_filters, window, mel, mel_batch_stride, mel_row_stride, workspace, workspace_bytes,
                           stream);
}

extern "C" int la_logmel_f32_prepared(const float *audio, int32_t batch, int32_t n_samples, const void *consts, float *mel,
                                      int64_t mel_batch_stride, int64_t mel_row_stride, void *workspace, size_t workspace_bytes, void *stream) {
    return la_logmel_f32_prepared_n(80, audio, batch, n_samples, consts, mel, mel_batch_stride, mel_row_stride, workspace, workspace_bytes,
                                    stream);
}

extern "C" int la_logmel_ragged_workspace_bytes(int32_t batch, int32_t max_samples, size_t *bytes) {
    LA_CHECK_ARG(bytes && batch > 0 && max_samples >= HOP, "logmel_ragged_workspace_bytes: bad arguments");
    return la_logmel_workspace_bytes_n(80, batch, max_samples, bytes);
}

extern "C" int la_logmel_ragged_f32_prepared(const float *audio, const int32_t *n_samples, int32_t batch, int32_t max_samples, const void *consts,
                                             float *mel, int64_t mel_batch_stride, int64_t mel_row_stride, int32_t out_frames, void *workspace,
                                             size_t workspace_bytes, void *stream) {
    return la_logmel_ragged_f32_prepared_n(80, audio, n_samples, batch, max_samples, consts, mel, mel_batch_stride, mel_row_stride, out_frames,
                                           workspace, workspace_bytes, stream);
}

