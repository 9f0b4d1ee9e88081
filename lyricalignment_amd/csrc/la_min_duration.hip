// la_min_duration.hip -- the alignment DP on the plain lattice with a FLOOR on every character's duration (gfx950).
//
// States as in la_viterbi.hip: 0 = leading silence, 2n+1 = label n, 2n+2 = the silence after it, S = 2L+1.  min_frames[n] = D_n in
// 1 .. max_min_frames (<= 8) is the least number of frames a visit to label n lasts.  Label n carries D_n - 1 YOUNG values y_1 ..
// y_{D-1} (y_j: "in its j-th frame") and one MATURE value m ("has lasted at least D_n frames"); only m is visible to its successors.
//   row 0: dp[0][0] = em[0][0]; label 0: m = em[0][1] if D_0 == 1, else y_1 = em[0][1] and m = kNeg; every other value kNeg.
//   row t (reads row t-1 only; out_n = m_n[t-1], sil_i = state 2i, can_skip = n >= 1 && labels[n] != labels[n-1]):
//       state 0 stays; silence 2n+2 stays iff sil_{n+1}[t-1] > out_n (strict), else it comes from out_n;
//       label n with D_n == 1: la_viterbi.hip's choose_neighbour(p0 = m_n[t-1], p1 = sil_n[t-1], p2 = out_{n-1}, can_skip);
//       label n with D_n >= 2: entry = p2 if can_skip && p2 >= p1 else p1 (no stay candidate); y_1[t] = entry + em;
//           y_j[t] = y_{j-1}[t-1] + em (j = 2 .. D-1); m[t] = (m[t-1] > y_{D-1}[t-1] ? m[t-1] : y_{D-1}[t-1]) + em.
//   termination: start at 2L iff sil_L[T-1] > m_{L-1}[T-1] (strict), else at the last label's mature value: the last visit reaches
//       its floor too.  final_score is that value.
//   backtrace: a mature cell that GRADUATED at frame t puts the label on frames t-D+1 .. t and goes on from that first frame's entry
//       code.  LA_OK iff it arrives at frame 0 in state 0 or in the first frame of label 0; else LA_EINFEASIBLE with every onset /
//       offset / path entry -1 (final_score is still written).  A floor outside 1 .. max_min_frames among a clip's L_b entries:
//       LA_EINVAL for that clip.
// Everything is float64, the emission added last.
//
// Mapping: the tile form of la_lattice_tile.h.  What is this file's: THE YOUNG CHAIN of an odd state lives in DM - 1 float64 registers of
// the thread that owns the state and never crosses a thread; only m goes into the exchanged row.  The chain is kept RIGHT-ALIGNED --
// y_j in slot DM - D + j - 1 -- so that y_{D-1}, the one value m reads, is always the last slot and no slot is indexed at run time: per
// frame every slot takes its left neighbour (slot DM - D the entry instead) plus the emission, off the loop-carried chain of m.  Slots
// left of DM - D hold values that never reach a slot that is read.  DM (2, 4 or 8) is the smallest depth >= max_min_frames.
// Backpointers: three mask words -- the two-bit code of the entry (D >= 2) or of the cell (D == 1, silences), and THE GRADUATE BIT --
// and THE BACKTRACE that takes a visit at once.
#include "la_lattice_tile.h"

namespace {

using namespace la::lattice;

constexpr int kMaxFloor = 8;              // frames: the deepest chain built

struct FloorParams : LatticeIn {
    int32_t *onset, *offset;
    int32_t out_stride;
    double *final_score;
    int32_t *status;
    const int32_t *min_frames;            // [batch][mf_stride], entries 0 .. L_b - 1 of row b are read
    int32_t mf_stride;
    int32_t max_min_frames;
    int32_t *path;                        // [batch][path_stride]; null = not wanted
    int32_t path_stride;
    unsigned long long *bt;               // [batch][max_frames][R][NW][3]
};

template <int NW, int R, int DM>
__global__ __launch_bounds__(NW * 64) void viterbi_min_duration_kernel(FloorParams p) {
    static_assert(R == 1 || NW == 16, "several states per thread: the 1024-thread form");
    static_assert(DM >= 2 && DM <= kMaxFloor, "chain depth");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NT = NW * 64, NS = NT * R;
    constexpr bool ONE_WAVE = NW == 1;                      // (R = 1) neighbours by DPP
    constexpr int SPF = R == 1 ? 8 : R == 8 ? 2 : 4;        // emission prefetch depth (frames)
    constexpr int NODD = R == 1 ? 1 : R / 2;                // chains per thread (R = 1: the thread's one state, used where it is odd)
    constexpr int NY = DM - 1;                              // young slots per chain
    double *rowbuf = reinterpret_cast<double *>(smem);      // [2][NS + 2]
    __shared__ int infeasible;
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int L = p.n_labels[b];
    const int T = p.n_frames[b];
    const int S = 2 * L + 1;
    int32_t *on_g = p.onset + (int64_t)b * p.out_stride, *off_g = p.offset + (int64_t)b * p.out_stride;
    for (int n = tid; n < p.max_labels; n += NT) { on_g[n] = -1; off_g[n] = -1; }
    int32_t *path_b = nullptr;   // every frame -1 until the backtrace has been there
    if (p.path) {
        path_b = p.path + (int64_t)b * p.path_stride;
        for (int t = tid; t < p.max_frames; t += NT) path_b[t] = -1;
    }
    if (L <= 0) {
        if (tid == 0) { p.status[b] = LA_EEMPTY; p.final_score[b] = 0.0; }
        return;
    }
    if (T <= 0 || T > p.max_frames || L > p.max_labels || S > NS) {
        if (tid == 0) { p.status[b] = LA_EINVAL; p.final_score[b] = 0.0; }
        return;
    }
    const int32_t *mf = p.min_frames + (int64_t)b * p.mf_stride;
    {   // every floor of the clip inside 1 .. max_min_frames (<= DM), by the whole workgroup
        bool bad = false;
        for (int n = tid; n < L; n += NT) bad |= mf[n] < 1 || mf[n] > p.max_min_frames;
        if (__syncthreads_or(bad)) {
            if (tid == 0) { p.status[b] = LA_EINVAL; p.final_score[b] = 0.0; }
            return;
        }
    }
    unsigned long long *bt = p.bt + (int64_t)b * p.max_frames * (R * NW * 3);
    const int32_t *lab = p.labels + (int64_t)b * p.labels_stride;
    const float *emb = p.em + (int64_t)b * p.em_bs;
    const int k0 = tid * R;
    // what each owned state is: its emission column, whether the skip arc exists, its floor (1 for a silence), its chain
    int col[R], first[R];                   // first: the slot that takes the entry, DM - D (NY, i.e. no slot, where D == 1)
    bool can_skip[R], multi[R];
    double cur[R];
    double y[NODD][NY];
#pragma unroll
    for (int c = 0; c < NODD; ++c)
#pragma unroll
        for (int i = 0; i < NY; ++i) y[c][i] = kNeg;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int k = k0 + r, n = k >> 1;
        const bool valid = k < S, odd = (k & 1) != 0;
        col[r] = (odd && valid) ? 1 + n : 0;
        can_skip[r] = odd && valid && k >= 3 && lab[n] != lab[n - 1];
        const int D = (odd && valid) ? mf[n] : 1;
        multi[r] = D >= 2;
        first[r] = DM - D;
        cur[r] = k <= 1 ? (double)emb[col[r]] : kNeg;
        if (k == 1 && D >= 2) {             // row 0 of label 0: its first frame is young
#pragma unroll
            for (int i = 0; i < NY; ++i)
                if (i == first[r]) y[R == 1 ? 0 : r >> 1][i] = cur[r];
            cur[r] = kNeg;
        }
    }
    if (!ONE_WAVE && tid == 0) { rowbuf[0] = kNeg; rowbuf[1] = kNeg; rowbuf[NS + 2] = kNeg; rowbuf[NS + 3] = kNeg; }

    float e_buf[SPF][R];
#pragma unroll
    for (int i = 0; i < SPF; ++i)
#pragma unroll
        for (int r = 0; r < R; ++r) e_buf[i][r] = (1 + i) < T ? emb[(int64_t)(1 + i) * p.em_rs + col[r]] : 0.0f;
    int parity = 0;
    for (int j0 = 1; j0 < T; j0 += SPF) {
        float e_cur[SPF][R];
#pragma unroll
        for (int i = 0; i < SPF; ++i)
#pragma unroll
            for (int r = 0; r < R; ++r) e_cur[i][r] = e_buf[i][r];
#pragma unroll
        for (int i = 0; i < SPF; ++i)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int jj = j0 + SPF + i;
                e_buf[i][r] = jj < T ? emb[(int64_t)jj * p.em_rs + col[r]] : 0.0f;
            }
#pragma unroll
        for (int i = 0; i < SPF; ++i) {
            const int j = j0 + i;
            if (j >= T) break;
            double prev[R + 2];
            if constexpr (ONE_WAVE) {
                prev[1] = wave_shr1(cur[0], 0.0);      // (lane 0 is state 0: its neighbours are never chosen)
                prev[0] = wave_shr1(prev[1], 0.0);
            } else {
                double *rb = rowbuf + parity * (NS + 2);
                // the two rightmost states of this thread are the k-1 / k-2 neighbours of the next thread's first states
                rb[k0 + 2 + R - 1] = cur[R - 1];
                if constexpr (R >= 2) rb[k0 + 2 + R - 2] = cur[R - 2];
                __syncthreads();
                prev[0] = rb[k0];
                prev[1] = rb[k0 + 1];
                parity ^= 1;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) prev[r + 2] = cur[r];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double e = (double)e_cur[i][r];
                const double p0 = prev[r + 2], p1 = prev[r + 1], p2 = prev[r];
                unsigned long long *row = bt + (((int64_t)j * R + r) * NW + wave) * 3;
                if (R == 1 || (r & 1)) {                // (decided at compile time: the loop is unrolled)
                    // (R = 1: a silence runs this with can_skip false and D = 1, which is its own rule)
                    double *yc = y[R == 1 ? 0 : r >> 1];
                    const Cell c = choose_neighbour(p0, p1, p2, can_skip[r], k0 + r == 0);
                    const bool via_skip = can_skip[r] && p2 >= p1;
                    const double entry = via_skip ? p2 : p1;
                    const double ylast = yc[NY - 1];
                    const bool stay_m = p0 > ylast;
                    const double best = multi[r] ? (stay_m ? p0 : ylast) : c.best;
                    const int code = multi[r] ? (via_skip ? 2 : 1) : c.code;
                    cur[r] = best + e;
#pragma unroll
                    for (int s = NY - 1; s >= 1; --s) yc[s] = (s == first[r] ? entry : yc[s - 1]) + e;
                    yc[0] = entry + e;
                    const unsigned long long m0 = __ballot(code & 1);
                    const unsigned long long m1 = __ballot((code >> 1) & 1);
                    const unsigned long long mg = __ballot(multi[r] && !stay_m);
                    if (lane == 0) { row[0] = m0; row[1] = m1; row[2] = mg; }
                } else {
                    const bool stay = p0 > p1 || k0 + r == 0;
                    cur[r] = (stay ? p0 : p1) + e;
                    const unsigned long long m0 = __ballot(!stay);
                    if (lane == 0) row[0] = m0;         // (a silence: its other two words are never read)
                }
            }
        }
    }

    // termination + backtrace by one thread; the masks were written by other waves of this workgroup: drain + barrier first
    __syncthreads();
    double *fin = rowbuf;
#pragma unroll
    for (int r = 0; r < R; ++r) fin[k0 + r] = cur[r];
    if (tid == 0) infeasible = 0;
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        int kk = (fin[S - 1] > fin[S - 2]) ? (S - 1) : (S - 2);   // strict '>' (:157)
        p.final_score[b] = fin[kk];
        auto bit = [&](int j, int k, int w) {
            const int t2 = k / R, r = k - t2 * R;
            return (int)((bt[(((int64_t)j * R + r) * NW + (t2 >> 6)) * 3 + w] >> (t2 & 63)) & 1ull);
        };
        bool ok = false;
        int j = T - 1, knext = -1;
        while (true) {
            const int n = kk >> 1;
            const int D = (kk & 1) ? mf[n] : 1;
            if (D >= 2) {
                // a mature cell: back to the frame at which the visit graduated, then the whole visit at once
                int t = j;
                while (t > 0 && !bit(t, kk, 2)) --t;
                const int f = t - D + 1;
                if (t == 0 || f < 0) break;            // mature at frame 0, or a visit that began before it
                off_g[n] = j + 1;
                on_g[n] = f;
                if (path_b)
                    for (int u = f; u <= j; ++u) path_b[u] = kk;
                if (f == 0) { ok = kk == 1; break; }
                knext = kk;
                kk -= bit(f, kk, 0) | (bit(f, kk, 1) << 1);
                j = f - 1;
            } else {
                if (path_b) path_b[j] = kk;
                if ((kk & 1) && kk != knext) off_g[n] = j + 1;   // last frame of this visit + 1
                if (j == 0) {
                    if (kk & 1) on_g[n] = 0;
                    ok = kk <= 1;
                    break;
                }
                const int code = bit(j, kk, 0) | ((kk & 1) ? bit(j, kk, 1) << 1 : 0);   // (a silence has one word)
                if ((kk & 1) && code != 0) on_g[n] = j;         // frame j is the first one of this visit
                knext = kk;
                kk -= code;
                --j;
            }
        }
        p.status[b] = ok ? LA_OK : LA_EINFEASIBLE;
        infeasible = !ok;
    }
    __threadfence_block();
    __syncthreads();
    if (infeasible) {   // no partial rows: every output of the clip is -1
        for (int n = tid; n < L; n += NT) { on_g[n] = -1; off_g[n] = -1; }
        if (path_b)
            for (int t = tid; t < T; t += NT) path_b[t] = -1;
    }
}

struct FloorPlan {
    Tile tile;
    int dm;
    size_t lds_bytes, ws_bytes;
};

bool plan_floor(int batch, int max_frames, int max_labels, int max_min_frames, FloorPlan *pl) {
    if (!plan_tile(max_labels, 4095, &pl->tile)) return false;
    pl->dm = max_min_frames <= 2 ? 2 : max_min_frames <= 4 ? 4 : 8;
    pl->lds_bytes = 2 * (size_t)(pl->tile.states() + 2) * sizeof(double);   // (one wave: the final row only)
    pl->ws_bytes = (size_t)batch * max_frames * pl->tile.r * pl->tile.nw * 3 * sizeof(unsigned long long);
    return true;
}

template <int DM>
int launch_depth(const FloorParams &p, const FloorPlan &pl, int batch, hipStream_t stream) {
    return for_tile(pl.tile, [&](auto nw, auto r) {
        constexpr int NW = decltype(nw)::value, R = decltype(r)::value;
        return launch<viterbi_min_duration_kernel<NW, R, DM>>("viterbi_min_duration", NW * 64, p, pl, batch, stream);
    });
}

}  // namespace

extern "C" int la_viterbi_min_duration_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, int32_t max_min_frames,
                                                       size_t *bytes) {
    LA_CHECK_ARG(bytes && batch >= 0 && max_frames > 0 && max_labels > 0, "viterbi_min_duration_workspace_bytes: bad arguments");
    LA_CHECK_ARG(max_min_frames >= 1 && max_min_frames <= kMaxFloor, "viterbi_min_duration_workspace_bytes: max_min_frames must be 1 .. %d",
                 kMaxFloor);
    FloorPlan pl;
    if (!plan_floor(batch, max_frames, max_labels, max_min_frames, &pl)) return over_label_limit("viterbi_min_duration", max_labels);
    *bytes = pl.ws_bytes;
    return LA_OK;
}

extern "C" int la_viterbi_min_duration_batch(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                                             const int32_t *labels, int32_t labels_stride, const int32_t *n_labels,
                                             const int32_t *n_frames, int32_t batch, int32_t max_frames, int32_t max_labels,
                                             int32_t *onset, int32_t *offset, int32_t out_stride, double *final_score,
                                             int32_t *status, const int32_t *min_frames, int32_t min_frames_stride, int32_t max_min_frames,
                                             int32_t *path, int32_t path_stride, void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "viterbi_min_duration_batch";
    if (batch == 0) return LA_OK;
    FloorParams p{};
    p.set_inputs(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels);
    LA_CHECK_ARG(p.inputs_present(Face::Plain) && min_frames && onset && offset && final_score && status, "%s: null pointer", who);
    LA_CHECK_ARG(p.sizes_ok(batch), "%s: bad sizes", who);
    LA_CHECK_ARG(max_min_frames >= 1 && max_min_frames <= kMaxFloor, "%s: max_min_frames must be 1 .. %d", who, kMaxFloor);
    FloorPlan pl;
    if (!plan_floor(batch, max_frames, max_labels, max_min_frames, &pl)) return over_label_limit("viterbi_min_duration", max_labels);
    LA_CHECK_ARG(p.strides_ok(Face::Plain, out_stride, false) && min_frames_stride >= max_labels, "%s: strides smaller than max_labels", who);
    if (const int rc = check_path_and_workspace(who, path != nullptr, path_stride, max_frames, workspace, workspace_bytes, pl.ws_bytes)) return rc;
    p.onset = onset, p.offset = offset, p.out_stride = out_stride, p.final_score = final_score, p.status = status;
    p.min_frames = min_frames, p.mf_stride = min_frames_stride, p.max_min_frames = max_min_frames;
    p.path = path, p.path_stride = path_stride;
    p.bt = reinterpret_cast<unsigned long long *>(workspace);
    hipStream_t stream = (hipStream_t)stream_;
    switch (pl.dm) {
        case 2: return launch_depth<2>(p, pl, batch, stream);
        case 4: return launch_depth<4>(p, pl, batch, stream);
    }
    return launch_depth<8>(p, pl, batch, stream);
}
