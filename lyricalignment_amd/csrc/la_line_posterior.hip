// la_line_posterior.hip -- confidence for free line order: forward-backward (sum-product) on the lattice of la_line_order.hip (gfx950).
//
// States, jump sources, jump targets and the class rule are la_viterbi_lines_batch's (la_line_order.hip).  A path weighs exp(sum of its
// emissions) times one factor per transition: 1 for a plain one (k -> k, k -> k+1, k -> k+2 into an odd state whose neighbour label
// differs), q = exp(-penalty) for a jump (source -> target under the class rule, where the pair is not a plain transition already), 1 for a
// start in state 0 or 1 and q in any other target, 1 for an end in S-1 or S-2 and q in any other source but state 0.
//
// THE HUB, FOR SUMS.  With M lines the jumps are M^2 arcs.  Two things make them O(S + M) additions per frame, with nothing subtracted:
//   1. The jump term of a target 2a+1 runs over EVERY source the class rule allows, the plain duplicates 2a and (a >= 1, labels differ)
//      2a-1 included, at q; the plain advance and the plain skip INTO a line-start target weigh 1 - q instead of 1 (log_keep =
//      log(-expm1(-penalty)), taken once on the host in float64: -inf at penalty 0, 0 at +inf).  The pair then weighs exactly 1.
//      in_order counts those two arrivals at their full weight 1.
//   2. What remains is a leave-one-class-out sum: a target of class c takes the silence sources plus the odd sources of every class but c;
//      backward an odd source of class c takes q * beta_{t+1} of the targets of every class but c, a silence source all of them.  Once per
//      clip the kernel sorts the odd sources, and the targets, by (class, label index) -- a rank by counting over keys staged in LDS -- and
//      every thread keeps EPT consecutive positions of each sorted order.  Per frame the values at those positions go through one
//      exclusive prefix and one exclusive suffix scan (thread chunk, wave by shuffles, the waves' totals through LDS); the element that
//      begins a class group leaves the prefix before the group in the group's slot, the element that ends it adds the suffix after the
//      group and the silence total and leaves the logarithm there.  A query is one LDS read: the slot of its class (found once per clip by
//      binary search), or the plain total where its class has no group.
//   The scans run on pairs (s, e) that stand for s * 2^e -- a sum scaled to a power of two near its maximum: x -> (exp2(frac), floor)
//   of x / ln 2, combined by v_ldexp and one addition, so that a term any distance below the frame's largest keeps its full precision (a
//   fixed shift by the frame's best source would lose every term 708 nats below it).  Additions only, in an order fixed by the thread
//   layout: no atomics, the same bits from two calls and from a clip alone in the same kernel form.  All float64.
//
// Mapping: the tile form of la_lattice_tile.h, with ONE float64 row in LDS that carries alpha_{t-1} (backward: beta_{t+1}) of every
// state to the neighbours and to the hub; with the slots it is 130 KB at R = 8, so the row is not double-buffered: four barriers per
// frame.  What is this file's: THE XS SCALED SUMS, THE CLASS SORT and LEAVE_ONE_OUT.  Forward the alpha rows and every target's jump term
// go to the workspace; backward beta stays in registers, gamma and the per-label sums are formed by the thread that owns the state:
// visits and in_order in registers, the sparse ones (occupancy, onset, offset) in a slot of the workspace.  The neighbour terms of a step
// use la_lattice.h's log_add3 / log_add2 (float64 maximum, float32 correction), the jump terms log_add_jump (float64), as
// la_posterior.hip does.
#include "la_lattice_tile.h"

namespace {

using namespace la::lattice;

struct LinePostParams : LatticeIn {       // (penalty: the line jump's)
    const int32_t *onset, *offset;
    int32_t out_stride;
    int32_t window;
    const int32_t *line_start;            // [batch][line_stride], entries 0 .. L_b - 1 of row b are read
    int32_t line_stride;
    double log_keep;                      // log(1 - exp(-penalty))
    const int32_t *path;                  // [batch][path_stride]: the DP's state per frame; null = not given
    int32_t path_stride;
    float *occupancy, *onset_prob, *offset_prob, *visits, *in_order;   // [batch][out_stride]
    float *path_prob;                     // [batch][path_stride]; null = not wanted
    double *log_z;
    int32_t *status;
    float *gamma;
    int64_t gamma_bs, gamma_rs;
    double *alpha_ws;                     // [batch][max_frames][NS]
    double *jin_ws;                       // [batch][max_frames][NS / 2]: the jump term into label n's state at frame t
    double *acc_ws;                       // [batch][NS / 2][3]: occupancy, onset and offset sums of label n
};

// s * 2^e; s == 0 is the empty sum
struct XS {
    double s;
    int e, pad;
};
static_assert(sizeof(XS) == 16, "one 16-byte slot per sorted position");
constexpr int kEmpty = -(1 << 28);
__device__ __forceinline__ XS xs_empty() { return {0.0, kEmpty, 0}; }
__device__ __forceinline__ XS xs_of_log(double a) {
    if (a == -INFINITY) return xs_empty();
    const double x = a * 1.4426950408889634074, f = floor(x);
    return {exp2(x - f), (int)f, 0};
}
__device__ __forceinline__ XS xs_add(XS a, XS b) {
    const int e = max(a.e, b.e);
    return {ldexp(a.s, a.e - e) + ldexp(b.s, b.e - e), e, 0};
}
__device__ __forceinline__ double xs_log(XS p) { return p.s == 0.0 ? -INFINITY : ((double)p.e + log2(p.s)) * 0.69314718055994530942; }
__device__ __forceinline__ XS xs_up(XS p, int d) { return {__shfl_up(p.s, d), __shfl_up(p.e, d), 0}; }
__device__ __forceinline__ XS xs_down(XS p, int d) { return {__shfl_down(p.s, d), __shfl_down(p.e, d), 0}; }
__device__ __forceinline__ XS xs_xor(XS p, int d) { return {__shfl_xor(p.s, d), __shfl_xor(p.e, d), 0}; }

// (class, label index) in one ascending key; ~0 = not an element of this order
__device__ __forceinline__ unsigned long long sort_key(int cls, int n) {
    return ((unsigned long long)((unsigned)cls ^ 0x80000000u) << 32) | (unsigned)n;
}
// the first position of class c among n ascending classes, or -1
__device__ __forceinline__ int first_of_class(const int32_t *cls, int n, int c) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cls[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && cls[lo] == c ? lo : -1;
}

template <int NW, int R>
__global__ __launch_bounds__(NW * 64) void line_posterior_kernel(LinePostParams p) {
    static_assert(R == 1 || NW == 16, "several states per thread: the 1024-thread form");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NT = NW * 64, NS = NT * R, LC = NS / 2;   // LC: label capacity (L < LC)
    constexpr int EPT = (R + 1) / 2;                        // sorted positions per thread, and odd states per thread
    constexpr int NE = NT * EPT;
    // own state k at [k + 2]; [0], [1] and [NS + 2], [NS + 3] stay -inf: the neighbours of the first / last states
    double *row = reinterpret_cast<double *>(smem);                                    // [NS + 4]
    XS *slot = reinterpret_cast<XS *>(smem + (size_t)(NS + 4) * sizeof(double));       // [NE]
    XS *wtot = slot + NE;                                                              // [2][NW]: the waves' totals, their silence totals
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int L = p.n_labels[b];
    const int T = p.n_frames[b];
    const int S = 2 * L + 1;
    const int Sg = 2 * p.max_labels + 1;   // <= NS (planned from max_labels)
    const int k0 = tid * R;
    const double NEG = -INFINITY;

    float *occ_g = p.occupancy + (int64_t)b * p.out_stride;
    float *onp_g = p.onset_prob + (int64_t)b * p.out_stride;
    float *offp_g = p.offset_prob + (int64_t)b * p.out_stride;
    float *vis_g = p.visits + (int64_t)b * p.out_stride;
    float *ino_g = p.in_order + (int64_t)b * p.out_stride;
    float *gam = p.gamma ? p.gamma + (int64_t)b * p.gamma_bs : nullptr;
    float *pp_g = p.path_prob ? p.path_prob + (int64_t)b * p.path_stride : nullptr;
    auto zero_gamma_from = [&](int t_from) {
        if (gam)
            for (int t = t_from; t < p.max_frames; ++t)
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (k0 + r < Sg) gam[(int64_t)t * p.gamma_rs + k0 + r] = 0.f;
    };
    auto zero_path_prob_from = [&](int t_from) {
        if (pp_g)
            for (int t = t_from + tid; t < p.max_frames; t += NT) pp_g[t] = 0.f;
    };
    auto fail = [&](int st, double lz) {
        for (int n = tid; n < p.max_labels; n += NT) { occ_g[n] = 0.f; onp_g[n] = 0.f; offp_g[n] = 0.f; vis_g[n] = 0.f; ino_g[n] = 0.f; }
        zero_path_prob_from(0);
        zero_gamma_from(0);
        if (tid == 0) { p.status[b] = st; p.log_z[b] = lz; }
    };
    if (L <= 0) { fail(LA_EEMPTY, 0.0); return; }
    const int32_t *ls = p.line_start + (int64_t)b * p.line_stride;
    if (T <= 0 || T > p.max_frames || L > p.max_labels || S > NS || ls[0] == 0) { fail(LA_EINVAL, 0.0); return; }

    const int32_t *lab = p.labels + (int64_t)b * p.labels_stride;
    const float *emb = p.em + (int64_t)b * p.em_bs;
    const double pen = p.penalty, lk = p.log_keep;
    double *aw = p.alpha_ws + (int64_t)b * p.max_frames * NS;
    double *jw = p.jin_ws + (int64_t)b * p.max_frames * LC;
    double *acc = p.acc_ws + (int64_t)b * LC * 3;

    // what each owned state is (la_line_order.hip); into: it is a line-start target; to1 / to2: so is k+1 / k+2
    int col[R];
    bool can_skip[R], can_skip_from[R], src[R], tgt[R], to1[R], to2[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int k = k0 + r, n = k >> 1;
        const bool valid = k < S, odd = (k & 1) != 0;
        col[r] = (odd && valid) ? 1 + n : 0;
        can_skip[r] = odd && valid && k >= 3 && lab[n] != lab[n - 1];            // k-2 -> k
        can_skip_from[r] = odd && valid && (k + 2 < S) && lab[n + 1] != lab[n];  // k -> k+2
        const int e = odd ? n + 1 : n;                          // the line end this state would close: 2e-1 (odd) or 2e (even)
        src[r] = valid && (k == 0 || e == L || ls[e] != 0);
        tgt[r] = odd && valid && ls[n] != 0;
        to1[r] = !odd && k + 1 < S && ls[n] != 0;               // k+1 = 2n+1
        to2[r] = odd && k + 2 < S && ls[n + 1] != 0;            // k+2 = 2(n+1)+1
    }

    // ---- once per clip: the odd sources and the targets, each sorted by (class, label index) ----------------------------------------
    int n_src = 0, n_tgt = 0;              // how many there are
    int el_s[EPT], el_t[EPT];              // the label at sorted position tid * EPT + j of either order, -1 past its end
    int gs_s[EPT], gs_t[EPT];              // where that label's class group begins, if the label ENDS the group; else -1
    bool st_s[EPT], st_t[EPT];             // the label BEGINS its class group
    int q_f[EPT], q_b[EPT];                // per owned odd state: the slot of its class among the sources / the targets, -1 = no group
    {
        unsigned long long *key_s = reinterpret_cast<unsigned long long *>(slot), *key_t = key_s + LC;   // 16 LC <= 16 NE bytes
        int32_t *perm_s = reinterpret_cast<int32_t *>(row), *perm_t = perm_s + LC;                       // 16 LC <= 8 NS bytes
        int32_t *cls_s = perm_t + LC, *cls_t = cls_s + LC;
        for (int n = tid; n < LC; n += NT) {
            const bool in = n < L;
            const int c = in ? lab[n] : 0;
            key_s[n] = in && (n + 1 == L || ls[n + 1] != 0) ? sort_key(c, n) : ~0ull;
            key_t[n] = in && ls[n] != 0 ? sort_key(c, n) : ~0ull;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < EPT; ++j) {   // label n's rank in either order: the keys below its own (uniform loop, broadcast reads)
            const int n = tid + j * NT;
            const unsigned long long ks = n < L ? key_s[n] : ~0ull, kt = n < L ? key_t[n] : ~0ull;
            int rs = 0, rt = 0, cs = 0, ct = 0;
            for (int m = 0; m < L; ++m) {
                const unsigned long long a = key_s[m], c = key_t[m];
                rs += a < ks; rt += c < kt;
                cs += a != ~0ull; ct += c != ~0ull;
            }
            n_src = cs, n_tgt = ct;
            if (ks != ~0ull) { perm_s[rs] = n; cls_s[rs] = lab[n]; }
            if (kt != ~0ull) { perm_t[rt] = n; cls_t[rt] = lab[n]; }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int i = tid * EPT + j;
            el_s[j] = el_t[j] = gs_s[j] = gs_t[j] = -1;
            st_s[j] = st_t[j] = false;
            if (i < n_src) {
                const int c = cls_s[i];
                el_s[j] = perm_s[i];
                st_s[j] = i == 0 || cls_s[i - 1] != c;
                if (i == n_src - 1 || cls_s[i + 1] != c) gs_s[j] = first_of_class(cls_s, n_src, c);
            }
            if (i < n_tgt) {
                const int c = cls_t[i];
                el_t[j] = perm_t[i];
                st_t[j] = i == 0 || cls_t[i - 1] != c;
                if (i == n_tgt - 1 || cls_t[i + 1] != c) gs_t[j] = first_of_class(cls_t, n_tgt, c);
            }
            // the owned odd state of index j: R = 1: the thread's only state; else r = 2 j + 1
            const int r = R == 1 ? 0 : 2 * j + 1;
            const int k = k0 + r;
            q_f[j] = q_b[j] = -1;
            if ((k & 1) && k < S) {
                const int c = lab[k >> 1];
                if (tgt[r]) q_f[j] = first_of_class(cls_s, n_src, c);
                if (src[r]) q_b[j] = first_of_class(cls_t, n_tgt, c);
            }
        }
        __syncthreads();   // the staging areas become the row and the slots
    }
    if (tid < 2) { row[tid] = NEG; row[NS + 2 + tid] = NEG; }

    // The leave-one-class-out sums of one frame.  c[j]: this thread's values in sorted order; extra: what joins every sum (the silence
    // sources); gs / st: the group marks of that order.  Afterwards slot[g].s holds, for the group that begins at sorted position g, the
    // logarithm of everything but the group; -> the logarithm of everything.  Three barriers.
    auto leave_one_out = [&](const XS (&c)[EPT], XS extra, const int (&gs)[EPT], const bool (&st)[EPT]) {
        XS loc = c[0];
#pragma unroll
        for (int j = 1; j < EPT; ++j) loc = xs_add(loc, c[j]);
        XS pre = loc, suf = loc;      // inclusive scans over the wave's lanes
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const XS o = xs_up(pre, d), q = xs_down(suf, d);
            if (lane >= d) pre = xs_add(o, pre);
            if (lane + d < 64) suf = xs_add(suf, q);
        }
#pragma unroll
        for (int d = 32; d; d >>= 1) extra = xs_add(extra, xs_xor(extra, d));
        if (lane == 63) wtot[wave] = pre;
        if (lane == 0) wtot[NW + wave] = extra;
        XS before = xs_up(pre, 1), after = xs_down(suf, 1);     // exclusive
        if (lane == 0) before = xs_empty();
        if (lane == 63) after = xs_empty();
        __syncthreads();
        XS wpre = xs_empty(), wsuf = xs_empty(), ext = xs_empty();
        for (int w = 0; w < NW; ++w) {
            ext = xs_add(ext, wtot[NW + w]);
            if (w < wave) wpre = xs_add(wpre, wtot[w]);
        }
        for (int w = NW - 1; w > wave; --w) wsuf = xs_add(wtot[w], wsuf);
        const XS all = xs_add(xs_add(xs_add(wpre, wtot[wave]), wsuf), ext);
        XS run = xs_add(wpre, before);
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            if (st[j]) slot[tid * EPT + j] = run;
            run = xs_add(run, c[j]);
        }
        __syncthreads();
        run = xs_add(after, wsuf);
#pragma unroll
        for (int j = EPT - 1; j >= 0; --j) {
            if (gs[j] >= 0) slot[gs[j]].s = xs_log(xs_add(xs_add(slot[gs[j]], run), ext));
            run = xs_add(c[j], run);
        }
        __syncthreads();
        return xs_log(all);
    };
    // the hub of the alpha row in LDS: the odd sources in their sorted order, the silence source after each and (zero: with) state 0
    auto source_hub = [&](bool zero) {
        XS c[EPT], extra = xs_empty();
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            c[j] = xs_empty();
            if (el_s[j] >= 0) {
                c[j] = xs_of_log(row[2 * el_s[j] + 3]);
                extra = xs_add(extra, xs_of_log(row[2 * el_s[j] + 4]));
            }
        }
        if (zero && tid == 0) extra = xs_add(extra, xs_of_log(row[2]));
        return leave_one_out(c, extra, gs_s, st_s);
    };

    // ---- forward ----
    double cur[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int k = k0 + r;
        cur[r] = k <= 1 ? (double)emb[col[r]] : NEG;
        if (tgt[r] && k != 1) cur[r] = (double)emb[col[r]] - pen;
        aw[k] = cur[r];
    }
    for (int t = 1; t < T; ++t) {
        float e[R];
#pragma unroll
        for (int r = 0; r < R; ++r) e[r] = emb[(int64_t)t * p.em_rs + col[r]];
#pragma unroll
        for (int r = 0; r < R; ++r) row[k0 + r + 2] = cur[r];
        __syncthreads();
        double prev[R + 2];
        prev[0] = row[k0];
        prev[1] = row[k0 + 1];
#pragma unroll
        for (int r = 0; r < R; ++r) prev[r + 2] = cur[r];
        const double total = source_hub(true);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int k = k0 + r;
            const double w = tgt[r] ? lk : 0.0;
            double sum = log_add3(prev[r + 2], w + prev[r + 1], can_skip[r] ? w + prev[r] : NEG);
            if (tgt[r]) {
                const int q = q_f[R == 1 ? 0 : r >> 1];
                const double jin = (q >= 0 ? slot[q].s : total) - pen;
                jw[(int64_t)t * LC + (k >> 1)] = jin;
                sum = log_add_jump(sum, jin);
            }
            cur[r] = k < S ? sum + (double)e[r] : NEG;
            aw[(int64_t)t * NS + k] = cur[r];
        }
    }
    // log_z: S-1 and S-2 end at weight 1 = (1 - q) + q, every other source but state 0 at q
#pragma unroll
    for (int r = 0; r < R; ++r) row[k0 + r + 2] = cur[r];
    __threadfence_block();   // the backward sweep reads alpha columns written by other threads
    __syncthreads();
    const double log_z = log_add(log_add(lk + row[S + 1], lk + row[S]), source_hub(false) - pen);
    __syncthreads();         // (row is written again below)
    if (log_z == -INFINITY) { fail(LA_EINFEASIBLE, log_z); return; }

    // ---- backward: beta in registers ----
    int on[EPT], off[EPT];
    bool accl[EPT];
    double s_vis[EPT], s_ino[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int k = k0 + (R == 1 ? 0 : 2 * j + 1), n = k >> 1;
        on[j] = off[j] = -1;
        if ((k & 1) && k < S) { on[j] = p.onset[(int64_t)b * p.out_stride + n]; off[j] = p.offset[(int64_t)b * p.out_stride + n]; }
        accl[j] = on[j] >= 0 && off[j] > on[j];
        s_vis[j] = s_ino[j] = 0.0;
        if (k & 1) { acc[n * 3] = 0.0; acc[n * 3 + 1] = 0.0; acc[n * 3 + 2] = 0.0; }   // (n < LC)
    }
    const int32_t *path_b = pp_g ? p.path + (int64_t)b * p.path_stride : nullptr;   // (the host: path_prob only with a path)
    const int wnd = p.window;
    double be[R];
    for (int t = T - 1; t >= 0; --t) {
        float e[R];
#pragma unroll
        for (int r = 0; r < R; ++r) e[r] = emb[(int64_t)t * p.em_rs + col[r]];
        const int pc = path_b ? path_b[t] : -1;
        double out[R], js[R];
        if (t == T - 1) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int k = k0 + r;
                const double endw = (k == S - 1 || k == S - 2) ? 0.0 : (src[r] && k != 0 ? -pen : NEG);
                be[r] = k < S ? endw + (double)e[r] : NEG;
                out[r] = js[r] = NEG;
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) row[k0 + r + 2] = be[r];
            __syncthreads();
            double nb[R + 2];
#pragma unroll
            for (int r = 0; r < R; ++r) nb[r] = be[r];
            nb[R] = row[k0 + R + 2];
            nb[R + 1] = row[k0 + R + 3];
            XS c[EPT];
#pragma unroll
            for (int j = 0; j < EPT; ++j) c[j] = el_t[j] >= 0 ? xs_of_log(row[2 * el_t[j] + 3]) : xs_empty();
            const double total = leave_one_out(c, xs_empty(), gs_t, st_t);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int k = k0 + r;
                const double b1 = (to1[r] ? lk : 0.0) + nb[r + 1];
                const double b2 = can_skip_from[r] ? (to2[r] ? lk : 0.0) + nb[r + 2] : NEG;
                js[r] = NEG;
                if (src[r]) {
                    const int q = (k & 1) ? q_b[R == 1 ? 0 : r >> 1] : -1;
                    js[r] = (q >= 0 ? slot[q].s : total) - pen;
                }
                out[r] = log_add2(b1, b2);
                const double sum = log_add_jump(log_add3(nb[r], b1, b2), js[r]);
                be[r] = k < S ? sum + (double)e[r] : NEG;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int k = k0 + r, n = k >> 1;
            const double at = aw[(int64_t)t * NS + k];
            const float g = __expf((float)(at + be[r] - (double)e[r] - log_z));
            if (gam && k < Sg) gam[(int64_t)t * p.gamma_rs + k] = g;
            const bool named = pc >= 0 && pc < S;
            if (pp_g && k == (named ? pc : 0)) pp_g[t] = named ? g : 0.f;
            if ((k & 1) && k < S) {
                const int j = R == 1 ? 0 : r >> 1;
                float en = g, ino = (t == 0 && k == 1) ? g : 0.f;
                if (t > 0) {
                    const double *prow = aw + (int64_t)(t - 1) * NS + k;
                    const double am1 = prow[-1], am2 = can_skip[r] ? prow[-2] : NEG;
                    const double w = tgt[r] ? lk : 0.0;
                    double in = log_add2(w + am1, w + am2);
                    if (tgt[r]) {
                        in = log_add_jump(in, jw[(int64_t)t * LC + n]);
                        ino = __expf((float)(log_add2(am1, am2) + be[r] - log_z));
                    }
                    en = __expf((float)(in + be[r] - log_z));
                }
                s_vis[j] += (double)en;
                if (tgt[r]) s_ino[j] += (double)ino;
                if (accl[j]) {
                    if (t >= on[j] && t < off[j]) acc[n * 3] += (double)g;
                    if (abs(t - on[j]) <= wnd) acc[n * 3 + 1] += (double)en;
                    if (abs(t - (off[j] - 1)) <= wnd) {
                        const float ex = t == T - 1 ? g : __expf((float)(at + log_add_jump(out[r], js[r]) - log_z));
                        acc[n * 3 + 2] += (double)ex;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int k = k0 + (R == 1 ? 0 : 2 * j + 1), n = k >> 1;
        if (!(k & 1) || n >= p.max_labels) continue;
        const bool a = accl[j];
        occ_g[n] = a ? (float)(acc[n * 3] / (double)(off[j] - on[j])) : 0.f;
        onp_g[n] = a ? (float)acc[n * 3 + 1] : 0.f;
        offp_g[n] = a ? (float)acc[n * 3 + 2] : 0.f;
        vis_g[n] = k < S ? (float)s_vis[j] : 0.f;
        ino_g[n] = k < S ? (float)s_ino[j] : 0.f;
    }
    zero_path_prob_from(T);
    zero_gamma_from(T);
    if (tid == 0) { p.status[b] = LA_OK; p.log_z[b] = log_z; }
}

struct LinePostPlan {
    Tile tile;
    size_t lds_bytes, alpha_bytes, jin_bytes, ws_bytes;
};

bool plan_line_posterior(int batch, int max_frames, int max_labels, LinePostPlan *pl) {
    if (!plan_tile(max_labels, 4095, &pl->tile)) return false;
    const size_t nw = pl->tile.nw, nt = nw * 64, ns = pl->tile.states(), ept = (pl->tile.r + 1) / 2;
    pl->lds_bytes = (ns + 4) * sizeof(double) + nt * ept * sizeof(XS) + 2 * nw * sizeof(XS);
    pl->alpha_bytes = (size_t)batch * max_frames * ns * sizeof(double);
    pl->jin_bytes = (size_t)batch * max_frames * (ns / 2) * sizeof(double);
    pl->ws_bytes = pl->alpha_bytes + pl->jin_bytes + (size_t)batch * (ns / 2) * 3 * sizeof(double);
    return true;
}

}  // namespace

extern "C" int la_alignment_posteriors_lines_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    LA_CHECK_ARG(bytes && batch >= 0 && max_frames > 0 && max_labels > 0, "alignment_posteriors_lines_workspace_bytes: bad arguments");
    LinePostPlan pl;
    if (!plan_line_posterior(batch, max_frames, max_labels, &pl)) return over_label_limit("alignment_posteriors_lines", max_labels);
    *bytes = pl.ws_bytes;
    return LA_OK;
}

extern "C" int la_alignment_posteriors_lines(const float *em, int64_t em_batch_stride, int64_t em_row_stride, const int32_t *labels,
                                             int32_t labels_stride, const int32_t *n_labels, const int32_t *n_frames, int32_t batch,
                                             int32_t max_frames, int32_t max_labels, const int32_t *onset, const int32_t *offset,
                                             int32_t out_stride, int32_t boundary_window, const int32_t *line_start, int32_t line_stride,
                                             double line_jump_penalty, const int32_t *path, int32_t path_stride, float *occupancy,
                                             float *onset_prob, float *offset_prob, float *visits, float *in_order, float *path_prob,
                                             double *log_z, int32_t *status, float *gamma_out, int64_t gamma_batch_stride,
                                             int64_t gamma_row_stride, void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "alignment_posteriors_lines";
    if (batch == 0) return LA_OK;
    LinePostParams p{};
    p.set_inputs(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels);
    p.set_spans(nullptr, 0, line_jump_penalty);
    LA_CHECK_ARG(p.inputs_present(Face::Plain) && line_start && onset && offset, "%s: null input pointer", who);
    LA_CHECK_ARG(occupancy && onset_prob && offset_prob && visits && in_order && log_z && status, "%s: null output pointer", who);
    LA_CHECK_ARG(p.sizes_ok(batch), "%s: bad sizes", who);
    LA_CHECK_ARG(boundary_window >= 0, "%s: negative boundary_window", who);
    LA_CHECK_ARG(p.penalty_ok(Face::Spans), "%s: line_jump_penalty must be >= 0 (and not NaN)", who);
    LA_CHECK_ARG(!path_prob || path, "%s: path_prob needs the path it is asked about", who);
    LinePostPlan pl;
    if (!plan_line_posterior(batch, max_frames, max_labels, &pl)) return over_label_limit(who, max_labels);
    LA_CHECK_ARG(p.strides_ok(Face::Plain, out_stride, false) && line_stride >= max_labels, "%s: strides smaller than max_labels", who);
    LA_CHECK_ARG(!gamma_out || (gamma_row_stride >= 2 * (int64_t)max_labels + 1 &&
                                (batch == 1 || gamma_batch_stride >= (int64_t)max_frames * gamma_row_stride)),
                 "%s: gamma strides smaller than [max_frames][2 max_labels + 1]", who);
    if (const int rc = check_path_and_workspace(who, path || path_prob, path_stride, max_frames, workspace, workspace_bytes, pl.ws_bytes)) return rc;
    p.onset = onset, p.offset = offset, p.out_stride = out_stride, p.window = boundary_window;
    p.line_start = line_start, p.line_stride = line_stride;
    p.log_keep = log(-expm1(-line_jump_penalty));
    p.path = path, p.path_stride = path_stride;
    p.occupancy = occupancy, p.onset_prob = onset_prob, p.offset_prob = offset_prob, p.visits = visits, p.in_order = in_order;
    p.path_prob = path_prob, p.log_z = log_z, p.status = status;
    p.gamma = gamma_out, p.gamma_bs = gamma_batch_stride, p.gamma_rs = gamma_row_stride;
    unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
    p.alpha_ws = reinterpret_cast<double *>(ws);
    p.jin_ws = reinterpret_cast<double *>(ws + pl.alpha_bytes);
    p.acc_ws = reinterpret_cast<double *>(ws + pl.alpha_bytes + pl.jin_bytes);
    return for_tile(pl.tile, [&](auto nw, auto r) {
        constexpr int NW = decltype(nw)::value, R = decltype(r)::value;
        return launch<line_posterior_kernel<NW, R>>("posterior_lines", NW * 64, p, pl, batch, (hipStream_t)stream_);
    });
}
