// la_line_order.hip -- the alignment DP on the lattice of an UNMARKED lyric sheet: the lines may be sung in any order (gfx950).
//
// States as in la_viterbi.hip: 0 = leading silence, 2n+1 = label n, 2n+2 = the silence after it, S = 2L+1.  line_start[n] != 0 says that
// label n begins a line (entry 0 must).  After the last character of any line the path may go on to the first character of ANY line --
// the same one, an earlier one, or a later one with lines left out -- and it may begin at any line's start and stop at any line's end.
//   jump sources: state 0 and, for every line end e (the starts other than 0, and L), the states 2e-1 and 2e; the class of a source is
//       labels[s >> 1] for an odd state and "none" for a silence.
//   jump targets: the odd state 2a+1 of every line start a, from any source of frame t-1 whose class differs from labels[a] (the
//       equal-neighbour rule of repeat_source; a silence always differs).  Among the allowed sources the largest dp[t-1][s] wins, the
//       smallest index among equals; the jump is taken only if dp[t-1][s] - penalty is STRICTLY greater than choose_neighbour's winner.
//       The emission is added last.
//   free start: row 0 is the reference's, and every line start a != 0 gets em[0][1+a] - penalty.
//   free end: the reference's choice between S-1 and S-2 first; then the best source other than 0, S-1, S-2 (largest value, smallest
//       index) replaces it only if its value minus the penalty is strictly greater.
// With M lines these are M^2 arcs, but every arc carries the same penalty, so the best source of frame t-1 is the same for every target
// but those of its own class: per frame the kernel reduces the sources of row t-1 to THE HUB, two tuples (v1, s1, c1) -- the largest
// value, the smallest index among equals, its class -- and (v2, s2), the best source whose class differs from c1.  A target with
// labels[a] != c1 takes s1, any other target s2.  The work per frame does not depend on the number of lines.
//
// Mapping: the tile form of la_lattice_tile.h.  What is this file's: THE HUB REDUCTION -- every thread folds its own sources in registers,
// every wave reduces its lanes by a float64 maximum (four DPP steps inside a row of 16 lanes, the four rows by v_readlane), a ballot and a
// v_readlane of the winning lane's index, and lane 0 stores the wave's 32-byte partial beside the row BEFORE the frame's one barrier;
// after it lanes 0 .. NW-1 of every wave load the partials and fold them the same way (partials are double-buffered like the row; one
// wave keeps the hub in registers) -- THE CODE-3 JUMP -- backpointers are four codes {stay, advance, skip, hub jump}: two mask words,
// and s1 / s2 of every frame as two int32 behind the masks -- and THE BACKTRACE, which resolves a hub code by the same class compare.
// Everything is float64 in this order.
#include "la_lattice_tile.h"

namespace {

using namespace la::lattice;

constexpr int kNone = 0x7fffffff;         // "no source": larger than every state index, so a real source at -inf still wins the tie

struct LinesParams : LatticeIn {          // (penalty: the line jump's)
    int32_t *onset, *offset;
    int32_t out_stride;
    double *final_score;
    int32_t *status;
    const int32_t *line_start;            // [batch][line_stride], entries 0 .. L_b - 1 of row b are read
    int32_t line_stride;
    int32_t *path;                        // [batch][path_stride]; null = not wanted
    int32_t path_stride;
    unsigned long long *bt;               // [batch][max_frames][R][NW][2]
    int32_t *hub;                         // [batch][max_frames][2]: s1, s2 of the row before that frame
};

// the hub of one row, or one wave's part of it
struct Hub {
    double v1;
    int s1, c1;
    double v2;
    int s2, pad;
};
static_assert(sizeof(Hub) == 32, "one 32-byte partial per wave");

// Do state s (class c, read only where s is odd) and the hub's first source (s1, c1) have one class?  Two silences do ("none").
__device__ __forceinline__ bool same_class(int s, int c, int s1, int c1) { return (s & s1 & 1) ? c == c1 : !((s | s1) & 1); }

// the maximum over each row of 16 lanes, in every lane of the row: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror
__device__ __forceinline__ double row_max(double x) {
    x = fmax(x, dpp_f64<0xB1>(x));
    x = fmax(x, dpp_f64<0x4E>(x));
    x = fmax(x, dpp_f64<0x141>(x));
    return fmax(x, dpp_f64<0x140>(x));
}
// the maximum over the wave (ROWS = 4) or over its first row (ROWS = 1), wave-uniform
template <int ROWS>
__device__ __forceinline__ double wave_max(double x) {
    x = row_max(x);
    double m = readlane_f64(x, 0);
    if constexpr (ROWS == 4) m = fmax(fmax(m, readlane_f64(x, 16)), fmax(readlane_f64(x, 32), readlane_f64(x, 48)));
    return m;
}
// One (value, index, class) per lane, idx == kNone for a lane without one -> the largest value, the lowest lane among equals (lanes hold
// ascending state indices), wave-uniform.  idx stays kNone and the value -inf where no lane has one.
struct Top {
    double v;
    int s, c;
};
template <int ROWS>
__device__ __forceinline__ Top wave_top(double v, int idx, int cls) {
    const double m = wave_max<ROWS>(idx != kNone ? v : -INFINITY);
    const unsigned long long who = __ballot(idx != kNone && v == m);
    if (who == 0ull) return {-INFINITY, kNone, 0};
    const int f = __builtin_ctzll(who);
    return {m, __builtin_amdgcn_readlane(idx, f), __builtin_amdgcn_readlane(cls, f)};
}

template <int NW, int R>
__global__ __launch_bounds__(NW * 64) void viterbi_lines_kernel(LinesParams p) {
    static_assert(R == 1 || NW == 16, "several states per thread: the 1024-thread form");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NT = NW * 64, NS = NT * R;
    constexpr bool ONE_WAVE = NW == 1;                      // (R = 1) neighbours by DPP, the hub stays in registers
    constexpr int SPF = R == 1 ? 8 : R == 8 ? 2 : 4;        // emission prefetch depth (frames)
    double *rowbuf = reinterpret_cast<double *>(smem);                                      // [2][NS + 2]
    Hub *parts = reinterpret_cast<Hub *>(smem + 2 * (size_t)(NS + 2) * sizeof(double));     // [2][NW]
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
    const int32_t *ls = p.line_start + (int64_t)b * p.line_stride;
    if (T <= 0 || T > p.max_frames || L > p.max_labels || S > NS || ls[0] == 0) {   // (ls[0]: L >= 1 here)
        if (tid == 0) { p.status[b] = LA_EINVAL; p.final_score[b] = 0.0; }
        return;
    }
    unsigned long long *bt = p.bt + (int64_t)b * p.max_frames * (R * NW * 2);
    int32_t *hub_g = p.hub + (int64_t)b * p.max_frames * 2;
    const int32_t *lab = p.labels + (int64_t)b * p.labels_stride;
    const double pen = p.penalty;
    const float *emb = p.em + (int64_t)b * p.em_bs;
    const int k0 = tid * R;
    // what each owned state is: its emission column, its label (odd states), a jump source, a jump target
    int col[R], cls[R];
    bool can_skip[R], src[R], tgt[R];
    double cur[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int k = k0 + r, n = k >> 1;
        const bool valid = k < S, odd = (k & 1) != 0;
        col[r] = (odd && valid) ? 1 + n : 0;
        cls[r] = (odd && valid) ? lab[n] : 0;
        can_skip[r] = odd && valid && k >= 3 && lab[n] != lab[n - 1];
        const int e = odd ? n + 1 : n;                      // the line end this state would close: 2e-1 (odd) or 2e (even)
        src[r] = valid && (k == 0 || e == L || ls[e] != 0); // (valid: e <= L; ls is read below L only)
        tgt[r] = odd && valid && ls[n] != 0;
        // row 0: the reference's, and the free start
        cur[r] = k <= 1 ? (double)emb[col[r]] : kNeg;
        if (tgt[r] && n != 0) cur[r] = (double)emb[col[r]] - pen;
    }
    if (!ONE_WAVE && tid == 0) { rowbuf[0] = kNeg; rowbuf[1] = kNeg; rowbuf[NS + 2] = kNeg; rowbuf[NS + 3] = kNeg; }

    // The sources this thread owns, folded to one (value, index, class): the largest value, the smallest index among equals.
    // skip_s1: leave out the sources of (s1, c1)'s class (the hub's second tuple); END: leave out 0, S-1 and S-2 (the free end).
    auto own_top = [&](bool skip_s1, int s1, int c1, bool end) {
        Top t{-INFINITY, kNone, 0};
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int k = k0 + r;
            bool ok = src[r];
            if (skip_s1) ok = ok && !same_class(k, cls[r], s1, c1);
            if (end) ok = ok && k != 0 && k < S - 2;
            if (ok && (t.s == kNone || cur[r] > t.v)) t = {cur[r], k, cls[r]};
        }
        return t;
    };
    // this wave's part of the hub of the row in cur[]
    auto wave_hub = [&]() {
        const Top a = own_top(false, 0, 0, false);
        const Top t1 = wave_top<4>(a.v, a.s, a.c);
        const Top c = own_top(true, t1.s, t1.c, false);
        const Top t2 = wave_top<4>(c.v, c.s, c.c);
        return Hub{t1.v, t1.s, t1.c, t2.v, t2.s, 0};
    };
    // the NW partials of one row -> its hub, in every thread
    auto fold_parts = [&](const Hub *part) {
        Hub q{-INFINITY, kNone, 0, -INFINITY, kNone, 0};
        if (lane < NW) q = part[lane];
        const Top t1 = wave_top<1>(q.v1, q.s1, q.c1);
        // what a part has to offer beside the winner: its first source unless that one has the winner's class, then its second
        const bool second = same_class(q.s1, q.c1, t1.s, t1.c);
        const Top t2 = wave_top<1>(second ? q.v2 : q.v1, second ? q.s2 : q.s1, 0);
        return Hub{t1.v, t1.s, t1.c, t2.v, t2.s, 0};
    };

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
            Hub h = wave_hub();
            if constexpr (ONE_WAVE) {
                prev[1] = wave_shr1(cur[0], 0.0);      // (lane 0 is state 0: its neighbours are never chosen)
                prev[0] = wave_shr1(prev[1], 0.0);
            } else {
                double *rb = rowbuf + parity * (NS + 2);
                // the two rightmost states of this thread are the k-1 / k-2 neighbours of the next thread's first states
                rb[k0 + 2 + R - 1] = cur[R - 1];
                if constexpr (R >= 2) rb[k0 + 2 + R - 2] = cur[R - 2];
                Hub *part = parts + parity * NW;
                if (lane == 0) part[wave] = h;
                __syncthreads();
                prev[0] = rb[k0];
                prev[1] = rb[k0 + 1];
                h = fold_parts(part);
                parity ^= 1;
            }
            if (tid == 0) { hub_g[2 * j] = h.s1; hub_g[2 * j + 1] = h.s2; }
#pragma unroll
            for (int r = 0; r < R; ++r) prev[r + 2] = cur[r];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                Cell c = choose_neighbour(prev[r + 2], prev[r + 1], prev[r], can_skip[r], k0 + r == 0);
                if (tgt[r]) {
                    // (a target is an odd state: its class equals the first source's only where that one is a label)
                    const double v = ((h.s1 & 1) && h.c1 == cls[r] ? h.v2 : h.v1) - pen;
                    if (v > c.best) c = {3, v};
                }
                cur[r] = c.best + (double)e_cur[i][r];
                const unsigned long long m0 = __ballot(c.code & 1);
                const unsigned long long m1 = __ballot((c.code >> 1) & 1);
                if (lane == 0) {
                    unsigned long long *row = bt + (((int64_t)j * R + r) * NW + wave) * 2;
                    row[0] = m0;
                    row[1] = m1;
                }
            }
        }
    }

    // termination + backtrace by one thread; the masks were written by other waves of this workgroup: drain + barrier first
    __syncthreads();
    double *fin = rowbuf;
#pragma unroll
    for (int r = 0; r < R; ++r) fin[k0 + r] = cur[r];
    {   // the free end's candidate: each wave's best source other than 0, S-1 and S-2
        const Top a = own_top(false, 0, 0, true);
        const Top t = wave_top<4>(a.v, a.s, a.c);
        if (lane == 0) parts[wave] = Hub{t.v, t.s, 0, -INFINITY, kNone, 0};
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        int kk = (fin[S - 1] > fin[S - 2]) ? (S - 1) : (S - 2);   // strict '>' (:157)
        double score = fin[kk];
        int es = kNone;
        double ev = -INFINITY;
        for (int w = 0; w < NW; ++w)
            if (parts[w].s1 != kNone && (es == kNone || parts[w].v1 > ev)) { ev = parts[w].v1; es = parts[w].s1; }
        if (es != kNone && ev - pen > score) { kk = es; score = ev - pen; }
        p.final_score[b] = score;
        int knext = -1;
        for (int j = T - 1; j >= 0; --j) {
            if (path_b) path_b[j] = kk;
            if ((kk & 1) && kk != knext) off_g[kk >> 1] = j + 1;   // last frame of this visit + 1; an earlier visit overwrites a later one
            int knew = kk;
            if (j > 0) {
                const int t2 = kk / R, r = kk - t2 * R;
                const unsigned long long *row = bt + (((int64_t)j * R + r) * NW + (t2 >> 6)) * 2;
                const int sh = t2 & 63;
                const int code = (int)((row[0] >> sh) & 1ull) | ((int)((row[1] >> sh) & 1ull) << 1);
                if (code == 3) {
                    const int s1 = hub_g[2 * j];
                    knew = (s1 & 1) && lab[s1 >> 1] == lab[kk >> 1] ? hub_g[2 * j + 1] : s1;
                } else {
                    knew = kk - code;
                }
            }
            if ((kk & 1) && (j == 0 || knew != kk)) on_g[kk >> 1] = j;   // frame j is the first one of this visit
            knext = kk;
            kk = knew;
        }
        p.status[b] = LA_OK;   // (a label never visited keeps -1: lines may be left out)
    }
}

struct LinesPlan {
    Tile tile;
    size_t lds_bytes, bt_bytes, ws_bytes;   // bt_bytes: the masks of the whole batch, in front of the hub indices
};

bool plan_lines(int batch, int max_frames, int max_labels, LinesPlan *pl) {
    if (!plan_tile(max_labels, 4095, &pl->tile)) return false;
    const int nw = pl->tile.nw, r = pl->tile.r;
    pl->lds_bytes = 2 * (size_t)(pl->tile.states() + 2) * sizeof(double) + 2 * (size_t)nw * sizeof(Hub);   // (one wave: the final row only)
    pl->bt_bytes = (size_t)batch * max_frames * r * nw * 2 * sizeof(unsigned long long);
    pl->ws_bytes = pl->bt_bytes + (size_t)batch * max_frames * 2 * sizeof(int32_t);
    return true;
}

}  // namespace

extern "C" int la_viterbi_lines_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    LA_CHECK_ARG(bytes && batch >= 0 && max_frames > 0 && max_labels > 0, "viterbi_lines_workspace_bytes: bad arguments");
    LinesPlan pl;
    if (!plan_lines(batch, max_frames, max_labels, &pl)) return over_label_limit("viterbi_lines", max_labels);
    *bytes = pl.ws_bytes;
    return LA_OK;
}

extern "C" int la_viterbi_lines_batch(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                                      const int32_t *labels, int32_t labels_stride, const int32_t *n_labels,
                                      const int32_t *n_frames, int32_t batch, int32_t max_frames, int32_t max_labels,
                                      int32_t *onset, int32_t *offset, int32_t out_stride, double *final_score,
                                      int32_t *status, const int32_t *line_start, int32_t line_stride, double line_jump_penalty,
                                      int32_t *path, int32_t path_stride, void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "viterbi_lines_batch";
    if (batch == 0) return LA_OK;
    LinesParams p{};
    p.set_inputs(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels);
    p.set_spans(nullptr, 0, line_jump_penalty);
    LA_CHECK_ARG(p.inputs_present(Face::Plain) && line_start && onset && offset && final_score && status, "%s: null pointer", who);
    LA_CHECK_ARG(p.sizes_ok(batch), "%s: bad sizes", who);
    LA_CHECK_ARG(p.penalty_ok(Face::Spans), "%s: line_jump_penalty must be >= 0 (and not NaN)", who);
    LinesPlan pl;
    if (!plan_lines(batch, max_frames, max_labels, &pl)) return over_label_limit("viterbi_lines", max_labels);
    LA_CHECK_ARG(p.strides_ok(Face::Plain, out_stride, false) && line_stride >= max_labels, "%s: strides smaller than max_labels", who);
    if (const int rc = check_path_and_workspace(who, path != nullptr, path_stride, max_frames, workspace, workspace_bytes, pl.ws_bytes)) return rc;
    p.onset = onset, p.offset = offset, p.out_stride = out_stride, p.final_score = final_score, p.status = status;
    p.line_start = line_start, p.line_stride = line_stride;
    p.path = path, p.path_stride = path_stride;
    p.bt = reinterpret_cast<unsigned long long *>(workspace);
    p.hub = reinterpret_cast<int32_t *>(reinterpret_cast<unsigned char *>(workspace) + pl.bt_bytes);
    return for_tile(pl.tile, [&](auto nw, auto r) {
        constexpr int NW = decltype(nw)::value, R = decltype(r)::value;
        return launch<viterbi_lines_kernel<NW, R>>("viterbi_lines", NW * 64, p, pl, batch, (hipStream_t)stream_);
    });
}
