// la_posterior_strip.hip -- whole-song alignment confidence for gfx950: the sum-product sweep of la_posterior.hip on lattices
// beyond 1024 states (512 .. 4095 labels), and la_alignment_posteriors_lattice, the entry that takes any face at any size.
//
// posterior_strip_kernel<R, SPANS, WIN> is posterior_kernel's sweep on viterbi_strip_kernel's thread layout (la_viterbi.hip): one
// workgroup of 1024 threads per clip, thread tid owns the R CONSECUTIVE states k = tid*R + r (R = 2 / 4 / 8 -> 2048 / 4096 / 8192
// states).  Every cell is computed by the expression sequence of posterior_kernel -- log_add3 for the three-term step, log_add_jump
// for the jump terms in the same fixed order (J then J-1 forward, ascending target backward), the window's gate on the emission, the
// UNGATED emission in gamma -- so a clip gives the same bits here and there, and the error bound carries over (DESIGN.md
// "Whole-song posteriors").
//
// Forward: alpha rows go to the caller's workspace [batch][max_frames][1024 R] float64, a thread's R values as 16-byte pieces.
// Neighbours inside a thread are registers; the two rightmost states of a thread reach the next thread through a double-buffered
// float64 row in LDS, one barrier per frame.  Where the clip has a span (workgroup-uniform, tested once) every thread writes all R
// states into the row and reads alpha(J), alpha(J-1) from the row after the barrier, never from the registers the r loop overwrites.
// Backward: beta stays in registers; beta_{t+1}(k+1), (k+2) come from inside the thread or from the next thread's two leftmost
// states through the LDS row (with spans: the whole row, which the jump SOURCES read their targets from); alpha_{t-1}(k-1), (k-2)
// come from the thread's own prefetched alpha rows plus the two workspace values to its left; alpha_{t-1}(J), (J-1) from the workspace.
//
// What does not fit beside two full float64 rows (131,136 B of LDS at R = 8) lives elsewhere:
//   * the jump arcs by source (CSR) are built once per clip by the kernel -- skip_from staged in the not-yet-used row buffer, one pass
//     over the end positions for the count and one for the words -- into a per-thread list of (r, target) words in the caller's
//     workspace, ordered by r, then ascending target.  A thread folds its list front to back into js[r]: per state that is the
//     ascending-target order of posterior_kernel.  The first four words stay in registers; the trip count is the wave's maximum
//     list length;
//   * the sparse sums -- occupancy, onset, offset (a label adds to them only inside its segment or within boundary_window of a
//     boundary) and the span-skip mass (only a state where a span ends adds to it) -- are read-modify-written by the owning thread in
//     a slot of the workspace behind a divergent branch; present_prob, which every label of a clip with a span adds to at every frame,
//     stays in registers;
//   * states 2n and 2n+1 belong to the same thread (R is even), so span_skip_prob's final add needs no exchange.
// Both rows are double-buffered with one barrier per frame in both sweeps (DESIGN.md "Whole-song posteriors" has the budget).
#include <type_traits>

#include "la_lattice.h"

namespace {

using namespace la::lattice;

struct StripParams : LatticeIn {
    const int32_t *onset, *offset;
    int32_t out_stride;
    int32_t window;
    float *occupancy, *onset_prob, *offset_prob;
    double *log_z;
    int32_t *status;
    float *present_prob, *span_skip_prob;  // [batch][out_stride], [batch][skip_stride]
    float *gamma;
    int64_t gamma_bs, gamma_rs;
    double *alpha_ws;  // [batch][max_frames][1024 R]
    double *acc_ws;    // [batch][512 R][5]: occupancy, onset and offset sums of label n, span-skip sums of states 2n and 2n+1
    int32_t *csr_ws;   // [batch][2048 R]: jump arcs by source thread, (r << 16) | target
};

template <int R, bool SPANS, bool WIN>
__global__ __launch_bounds__(1024) void posterior_strip_kernel(StripParams p) {
    static_assert(!WIN || SPANS, "frame windows are a face of the optional-span forms");
    static_assert(R == 2 || R == 4 || R == 8, "states per thread");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NT = 1024, NS = NT * R, NL = R / 2, ROW = NS + 4;
    // frames per prefetch block (emissions, and backward the alpha rows): the span-free loops / the loops of a clip with a span
    constexpr int UP = R == 2 ? 4 : R == 4 ? 2 : 1, UJ = 1;
    constexpr int CR = 4;  // arc words kept in registers
    constexpr int AW = 5;  // sums per label kept in the workspace
    // own state k at [k + 2]; [0], [1] and [NS + 2], [NS + 3] stay -inf: the neighbours of the first / last states
    double *rowbuf = reinterpret_cast<double *>(smem);  // [2][ROW]
    double *fin = rowbuf + 2 * ROW;                     // [2]
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int L = p.n_labels[b];
    const int T = p.n_frames[b];
    const int S = 2 * L + 1;
    const int Sg = 2 * p.max_labels + 1;  // <= NS (planned from max_labels)
    const int k0 = tid * R, n0 = tid * NL;
    const double NEG = -INFINITY;

    float *occ_g = p.occupancy + (int64_t)b * p.out_stride;
    float *onp_g = p.onset_prob + (int64_t)b * p.out_stride;
    float *offp_g = p.offset_prob + (int64_t)b * p.out_stride;
    float *pres_g = p.present_prob + (int64_t)b * p.out_stride;
    float *skp_g = p.span_skip_prob + (int64_t)b * p.skip_stride;
    float *gam = p.gamma ? p.gamma + (int64_t)b * p.gamma_bs : nullptr;
    auto zero_gamma_from = [&](int t_from) {
        if (gam)
            for (int t = t_from; t < p.max_frames; ++t)
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (k0 + r < Sg) gam[(int64_t)t * p.gamma_rs + k0 + r] = 0.f;
    };
    auto fail = [&](int st, double lz) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int n = n0 + i;
            if (n < p.max_labels) { occ_g[n] = 0.f; onp_g[n] = 0.f; offp_g[n] = 0.f; pres_g[n] = 0.f; }
            if (n <= p.max_labels) skp_g[n] = 0.f;
        }
        zero_gamma_from(0);
        if (tid == 0) { p.status[b] = st; p.log_z[b] = lz; }
    };
    if (L <= 0) { fail(LA_EEMPTY, 0.0); return; }
    if (T <= 0 || T > p.max_frames || L > p.max_labels || S > NS) { fail(LA_EINVAL, 0.0); return; }

    const int32_t *lab = p.labels + (int64_t)b * p.labels_stride;
    bool can_skip[R], can_skip_from[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int k = k0 + r, n = k >> 1;
        const bool odd = (r & 1) != 0, valid = k < S;
        can_skip[r] = odd && valid && k >= 3 && lab[n] != lab[n - 1];            // k-2 -> k
        can_skip_from[r] = odd && valid && (k + 2 < S) && lab[n + 1] != lab[n];  // k -> k+2
    }
    // emission columns: [0] the blank of the even states, [1 + i] label n0 + i of the odd state 2 (n0 + i) + 1 (past the clip: the blank)
    const float *emb = p.em + (int64_t)b * p.em_bs;
    int col[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) col[i] = (k0 + 2 * i + 1 < S) ? 1 + n0 + i : 0;
    double *aw = p.alpha_ws + (int64_t)b * p.max_frames * NS;  // this clip's rows
    double *acc = p.acc_ws + ((int64_t)b * (NS / 2) + n0) * AW;  // this thread's labels

    // the span that ends at each owned state's position (la_lattice.h span_source), and each owned state's frame window
    [[maybe_unused]] const int32_t *skip_b = nullptr;
    [[maybe_unused]] int J[SPANS ? R : 1];
    [[maybe_unused]] bool jm1_ok[SPANS ? R : 1];
    [[maybe_unused]] int wlo[WIN ? R : 1], whi[WIN ? R : 1];
    bool has_span = false;
    if constexpr (SPANS) {
        if (!WIN || p.skip_from) skip_b = p.skip_from + (int64_t)b * p.skip_stride;  // (windows: a null skip_from = no span anywhere)
        bool any = false;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const SpanSource src = span_source(skip_b, lab, k0 + r, k0 + r < S);
            J[r] = src.J;
            jm1_ok[r] = src.jm1_ok;
            any |= src.J >= 0;
        }
        has_span = __syncthreads_or(any) != 0;  // workgroup-uniform, taken once: a clip without a span runs the plain loops
    }
    if constexpr (WIN) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            wlo[r] = 0, whi[r] = 0x7fffffff;
            if (k0 + r < S) {
                wlo[r] = p.win_lo[(int64_t)b * p.win_stride + k0 + r];
                whi[r] = p.win_hi[(int64_t)b * p.win_stride + k0 + r];
            }
        }
    }
    auto gated = [&](float e, int t, int r) {
        if constexpr (WIN) return (t >= wlo[r] && t < whi[r]) ? e : -INFINITY;
        else return e;
    };
    const double pen = p.penalty;

    // jump arcs by SOURCE: state k is J of the spans that start at position (k+1)/2 when even, J-1 of them when odd.  This thread's
    // list: tdeg words from csr[0], ordered by r, then ascending target
    int tdeg = 0, maxdeg = 0;
    [[maybe_unused]] int ent_reg[CR] = {0, 0, 0, 0};
    [[maybe_unused]] const int32_t *csr = nullptr;
    if constexpr (SPANS) {
        if (has_span) {
            int32_t *skip_s = reinterpret_cast<int32_t *>(rowbuf);      // [L + 1] <= 4 NS bytes
            int32_t *tot_s = reinterpret_cast<int32_t *>(rowbuf + ROW);  // [NT]
            for (int m = tid; m <= L; m += NT) skip_s[m] = span_first(skip_b, m);
            __syncthreads();
            // one pass over the end positions: a span (a, m) leaves from this thread's states 2a (always both targets) and 2a - 1
            // (the odd target only under the equal-neighbour rule), where they are its own: n0 <= a <= n0 + NL
            auto arcs = [&](auto emit) {
                for (int m = n0 + 1; m <= L; ++m) {
                    const int a = skip_s[m];
                    if (a < n0 || a > n0 + NL) continue;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int k = k0 + r;
                        if (((k + 1) >> 1) != a) continue;
                        const bool odd = (r & 1) != 0;
                        emit(r, 2 * m);
                        if (m < L && (!odd || lab[m] != lab[k >> 1])) emit(r, 2 * m + 1);  // the odd target 2m+1 besides 2m
                    }
                }
            };
            int cnt[R];
#pragma unroll
            for (int r = 0; r < R; ++r) cnt[r] = 0;
            arcs([&](int r, int) { ++cnt[r]; });
#pragma unroll
            for (int r = 0; r < R; ++r) tdeg += cnt[r];
            tot_s[tid] = tdeg;
            __syncthreads();
            int first = 0;
            for (int i = 0; i < NT; ++i) {  // uniform loop, broadcast reads
                const int v = tot_s[i];
                if (i < tid) first += v;
            }
            int32_t *mine = p.csr_ws + (int64_t)b * (2 * NS) + first;  // at most 4 arcs per span: < 2 NS in all
            int pos[R];                                                 // where the list of state r goes on: by r, then ascending target
            pos[0] = 0;
#pragma unroll
            for (int r = 1; r < R; ++r) pos[r] = pos[r - 1] + cnt[r - 1];
            arcs([&](int r, int d) { mine[pos[r]++] = (r << 16) | d; });
#pragma unroll
            for (int q = 0; q < CR; ++q) ent_reg[q] = q < tdeg ? mine[q] : 0;   // (written by this thread)
            csr = mine;
            maxdeg = tdeg;
            for (int o = 32; o; o >>= 1) maxdeg = max(maxdeg, __shfl_xor(maxdeg, o));
            maxdeg = __builtin_amdgcn_readfirstlane(maxdeg);
            __syncthreads();  // the row buffers are free again
        }
    }
    if (tid < 2) {
        rowbuf[tid] = NEG; rowbuf[ROW + tid] = NEG;
        rowbuf[NS + 2 + tid] = NEG; rowbuf[ROW + NS + 2 + tid] = NEG;
    }
#pragma unroll
    for (int i = 0; i < AW * NL; ++i) acc[i] = 0.0;
    __syncthreads();
    int parity = 0;

    // ---- forward: alpha_t(k) = e_t(k) + logsumexp(alpha_{t-1}(k), alpha_{t-1}(k-1), [alpha_{t-1}(k-2)]) ----
    double a[R];
    auto store_row = [&](int t) {
        double2 *dst = reinterpret_cast<double2 *>(aw + (int64_t)t * NS + k0);
#pragma unroll
        for (int i = 0; i < NL; ++i) dst[i] = make_double2(a[2 * i], a[2 * i + 1]);
    };
    {
        const float e0 = emb[0];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int k = k0 + r;
            a[r] = k <= 1 ? (double)gated(k == 0 ? e0 : emb[col[0]], 0, r) : NEG;
        }
        store_row(0);
    }
    auto forward = [&](auto has_c) {
        constexpr bool HAS = decltype(has_c)::value;  // this clip has a span
        constexpr int U = HAS ? UJ : UP;
        float ev[U][NL + 1];
        auto fetch = [&](int t0) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float *row = emb + (int64_t)min(t0 + u, T - 1) * p.em_rs;
                ev[u][0] = row[0];
#pragma unroll
                for (int i = 0; i < NL; ++i) ev[u][1 + i] = row[col[i]];
            }
        };
        fetch(1);
        for (int t0 = 1; t0 < T; t0 += U) {
            float ec[U][R];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int r = 0; r < R; ++r) ec[u][r] = gated((r & 1) ? ev[u][1 + (r >> 1)] : ev[u][0], t0 + u, r);  // off the dependent chain
            if (t0 + U < T) fetch(t0 + U);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u;
                if (t < T) {  // workgroup-uniform
                    double *rb = rowbuf + parity * ROW;
                    if constexpr (HAS) {
#pragma unroll
                        for (int r = 0; r < R; ++r) rb[k0 + 2 + r] = a[r];  // any state can be a jump source
                    } else {
                        rb[k0 + R] = a[R - 2];
                        rb[k0 + R + 1] = a[R - 1];
                    }
                    __syncthreads();
                    double prev[R + 2];
                    prev[0] = rb[k0];
                    prev[1] = rb[k0 + 1];
#pragma unroll
                    for (int r = 0; r < R; ++r) prev[r + 2] = a[r];
                    parity ^= 1;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const double a1 = prev[r + 1];
                        double a2 = prev[r];
                        if (!can_skip[r]) a2 = NEG;
                        double sum = log_add3(prev[r + 2], a1, a2);
                        if constexpr (HAS) {
                            if (J[r] >= 0) {  // from the row, never from a[]
                                const double aj = rb[J[r] + 2], ajm = rb[J[r] + 1];
                                sum = log_add_jump(sum, log_add_jump(aj - pen, jm1_ok[r] ? ajm - pen : NEG));
                            }
                        }
                        a[r] = k0 + r < S ? sum + (double)ec[u][r] : NEG;
                    }
                    store_row(t);
                }
            }
        }
    };
    if (has_span) forward(std::bool_constant<SPANS>{});
    else forward(std::false_type{});
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (k0 + r == S - 1) fin[0] = a[r];
        if (k0 + r == S - 2) fin[1] = a[r];
    }
    __threadfence_block();  // the backward sweep reads alpha values written by other threads
    __syncthreads();
    const double log_z = log_add(fin[0], fin[1]);
    if (log_z == -INFINITY) { fail(LA_EINFEASIBLE, log_z); return; }  // no path at all

    // ---- backward: beta in registers, gamma / entry / exit per step ----
    int on[NL], off[NL];
    bool acc_lane[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        on[i] = -1, off[i] = -1;
        if (k0 + 2 * i + 1 < S) { on[i] = p.onset[(int64_t)b * p.out_stride + n0 + i]; off[i] = p.offset[(int64_t)b * p.out_stride + n0 + i]; }
        acc_lane[i] = on[i] >= 0 && off[i] > on[i];
    }
    const int w = p.window;
    auto backward = [&](auto has_c) {
        constexpr bool HAS = decltype(has_c)::value;
        constexpr int U = HAS ? UJ : UP;
        // the next block's emissions and alpha rows are fetched while this block is computed, except where the clip has a span and
        // a thread owns 4 or 8 states: there the loads of a frame are issued at its start (the registers do not hold two generations)
        constexpr bool PF = !HAS || R == 2;
        [[maybe_unused]] double s_pres[HAS ? NL : 1];
        if constexpr (HAS) {
#pragma unroll
            for (int i = 0; i < NL; ++i) s_pres[i] = 0.0;
        }
        double be[R];
#pragma unroll
        for (int r = 0; r < R; ++r) be[r] = NEG;
        // alpha rows: `top` is alpha_t0 of the next block (carried, not fetched twice); nx[u] is row t0 - 1 - u, nl[u] the two values left of it
        double top[R], nx[U][R], nl[U][2];
        float ev[U][NL + 1];
        auto load_row = [&](double *dst, int t) {
            const double2 *src = reinterpret_cast<const double2 *>(aw + (int64_t)t * NS + k0);
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const double2 v = src[i];
                dst[2 * i] = v.x;
                dst[2 * i + 1] = v.y;
            }
        };
        auto fetch = [&](int t0) {  // steps t0, t0 - 1, ..., t0 - U + 1
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float *row = emb + (int64_t)max(t0 - u, 0) * p.em_rs;
                ev[u][0] = row[0];
#pragma unroll
                for (int i = 0; i < NL; ++i) ev[u][1 + i] = row[col[i]];
                const int tp = max(t0 - u - 1, 0);
                load_row(nx[u], tp);
                const double *left = aw + (int64_t)tp * NS + k0;
                nl[u][0] = tid > 0 ? left[-1] : NEG;
                nl[u][1] = tid > 0 ? left[-2] : NEG;
            }
        };
        load_row(top, T - 1);
        if constexpr (PF) fetch(T - 1);
        for (int t0 = T - 1; t0 >= 0; t0 -= U) {
            float ec[U][NL + 1];
            double ar[U + 1][R], al[U][2];
            if constexpr (!PF) fetch(t0);
#pragma unroll
            for (int r = 0; r < R; ++r) ar[0][r] = top[r];
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int i = 0; i <= NL; ++i) ec[u][i] = ev[u][i];
#pragma unroll
                for (int r = 0; r < R; ++r) ar[u + 1][r] = nx[u][r];
                al[u][0] = nl[u][0];
                al[u][1] = nl[u][1];
            }
#pragma unroll
            for (int r = 0; r < R; ++r) top[r] = ar[U][r];
            if constexpr (PF) {
                if (t0 - U >= 0) fetch(t0 - U);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 - u;
                if (t >= 0) {  // workgroup-uniform
                    double nb[R + 2];  // beta_{t+1} of the states k0 .. k0 + R + 1
                    [[maybe_unused]] double js[HAS ? R : 1];  // with spans: log weight of the jump arcs that leave each state
                    if (t != T - 1) {
                        double *rb = rowbuf + parity * ROW;
                        if constexpr (HAS) {
#pragma unroll
                            for (int r = 0; r < R; ++r) rb[k0 + 2 + r] = be[r];  // any state can be a jump target
                        } else {
                            rb[k0 + 2] = be[0];
                            rb[k0 + 3] = be[1];
                        }
                        __syncthreads();
#pragma unroll
                        for (int r = 0; r < R; ++r) nb[r] = be[r];
                        nb[R] = rb[k0 + R + 2];
                        nb[R + 1] = rb[k0 + R + 3];
                        parity ^= 1;
                        if constexpr (HAS) {  // fixed order: per state its targets, ascending
#pragma unroll
                            for (int r = 0; r < R; ++r) js[r] = NEG;
                            auto fold = [&](int i, int ent) {
                                const bool act = i < tdeg;
                                const int d = act ? (ent & 0xffff) : k0, er = ent >> 16;
                                const double bv = rb[d + 2];
                                double cur = js[0];
#pragma unroll
                                for (int r = 1; r < R; ++r) cur = er == r ? js[r] : cur;
                                const double res = log_add_jump(cur, bv - pen);
#pragma unroll
                                for (int r = 0; r < R; ++r) js[r] = (act && er == r) ? res : js[r];
                            };
#pragma unroll
                            for (int i = 0; i < CR; ++i)
                                if (i < maxdeg) fold(i, ent_reg[i]);
                            for (int i = CR; i < maxdeg; ++i) fold(i, i < tdeg ? csr[i] : 0);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int k = k0 + r;
                        const bool odd = (r & 1) != 0, valid = k < S;
                        const float ef = odd ? ec[u][1 + (r >> 1)] : ec[u][0];
                        const double e = (double)ef;
                        // gated in the sums, UNGATED in gamma's subtraction (depends on t and the prefetched value alone: off the chain)
                        const double eg = (double)gated(ef, t, r);
                        const double at = ar[u][r];
                        double out = NEG;  // log weight of leaving state k after frame t: beta_{t+1}(k+1), [beta_{t+1}(k+2)]
                        if (t == T - 1) {
                            be[r] = (k == S - 1 || k == S - 2) ? eg : NEG;
                            if constexpr (HAS) js[r] = NEG;
                        } else {
                            const double b1 = nb[r + 1];
                            double b2 = nb[r + 2];
                            if (!can_skip_from[r]) b2 = NEG;
                            out = log_add2(b1, b2);
                            double sum = log_add3(nb[r], b1, b2);
                            if constexpr (HAS) sum = log_add_jump(sum, js[r]);
                            be[r] = valid ? sum + eg : NEG;
                        }
                        // alpha_{t-1}(k-1), alpha_{t-1}(k-2)
                        const double am1 = r >= 1 ? ar[u + 1][r >= 1 ? r - 1 : 0] : al[u][0];
                        const double am2 = r >= 2 ? ar[u + 1][r >= 2 ? r - 2 : 0] : al[u][r == 0 ? 1 : 0];
                        [[maybe_unused]] double jin = NEG;  // with spans: log weight of the jump arcs into state k at frame t
                        if constexpr (HAS) {
                            if (J[r] >= 0 && t > 0) {
                                const double *prow = aw + (int64_t)(t - 1) * NS;
                                const double aj = prow[J[r]];
                                const double ajm = jm1_ok[r] ? prow[J[r] - 1] : NEG;
                                jin = log_add_jump(aj - pen, jm1_ok[r] ? ajm - pen : NEG);
                            }
                        }
                        const float g = __expf((float)(at + be[r] - e - log_z));  // alpha and beta both include e_t(k); outside a window both are -inf
                        if (gam && k < Sg) gam[(int64_t)t * p.gamma_rs + k] = g;
                        if constexpr (HAS) {
                            if (J[r] >= 0 && t > 0) acc[AW * (r >> 1) + 3 + (r & 1)] += (double)__expf((float)(jin + be[r] - log_z));
                            if (odd && valid) {
                                const int i = r >> 1;
                                float en = g;
                                if (t > 0) en = __expf((float)(log_add_jump(log_add2(am1, can_skip[r] ? am2 : NEG), jin) + be[r] - log_z));
                                s_pres[i] += (double)en;
                                if (acc_lane[i]) {
                                    if (t >= on[i] && t < off[i]) acc[AW * i] += (double)g;
                                    if (abs(t - on[i]) <= w) acc[AW * i + 1] += (double)en;
                                    if (abs(t - (off[i] - 1)) <= w) {
                                        const float ex = t == T - 1 ? g : __expf((float)(at + log_add_jump(out, js[r]) - log_z));
                                        acc[AW * i + 2] += (double)ex;
                                    }
                                }
                            }
                        } else if (odd) {
                            const int i = r >> 1;
                            if (acc_lane[i]) {
                                if (t >= on[i] && t < off[i]) acc[AW * i] += (double)g;
                                if (abs(t - on[i]) <= w) {
                                    float en = g;
                                    if (t > 0) en = __expf((float)(log_add2(am1, can_skip[r] ? am2 : NEG) + be[r] - log_z));
                                    acc[AW * i + 1] += (double)en;
                                }
                                if (abs(t - (off[i] - 1)) <= w) {
                                    const float ex = t == T - 1 ? g : __expf((float)(at + out - log_z));
                                    acc[AW * i + 2] += (double)ex;
                                }
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int n = n0 + i;
            const bool valid = k0 + 2 * i + 1 < S;
            if constexpr (HAS) {
                if (n < p.max_labels) pres_g[n] = valid ? (float)s_pres[i] : 0.f;
                if (n <= p.max_labels) skp_g[n] = J[2 * i] >= 0 ? (float)(acc[AW * i + 3] + acc[AW * i + 4]) : 0.f;  // states 2n and 2n+1
            } else {  // no jump: every path visits every label
                if (n < p.max_labels) pres_g[n] = valid ? 1.f : 0.f;
                if (n <= p.max_labels) skp_g[n] = 0.f;
            }
        }
    };
    if (has_span) backward(std::bool_constant<SPANS>{});
    else backward(std::false_type{});
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const int n = n0 + i;
        if (n < p.max_labels) {
            occ_g[n] = acc_lane[i] ? (float)(acc[AW * i] / (double)(off[i] - on[i])) : 0.f;
            onp_g[n] = acc_lane[i] ? (float)acc[AW * i + 1] : 0.f;
            offp_g[n] = acc_lane[i] ? (float)acc[AW * i + 2] : 0.f;
        }
    }
    zero_gamma_from(T);
    if (tid == 0) { p.status[b] = LA_OK; p.log_z[b] = log_z; }
}

// up to 511 labels and nothing given: la_alignment_posteriors wrote the five common outputs; the span outputs of a lattice without a
// span are what la_alignment_posteriors_spans gives for an all -1 skip_from
__global__ void no_span_outputs_kernel(const int32_t *status, const int32_t *n_labels, int32_t max_labels, float *present_prob,
                                       int32_t out_stride, float *span_skip_prob, int32_t skip_stride) {
    const int b = blockIdx.x;
    const int L = status[b] == LA_OK ? n_labels[b] : 0;
    for (int n = threadIdx.x; n <= max_labels; n += blockDim.x) {
        if (n < max_labels) present_prob[(int64_t)b * out_stride + n] = n < L ? 1.f : 0.f;
        span_skip_prob[(int64_t)b * skip_stride + n] = 0.f;
    }
}

const char kWho[] = "alignment_posteriors_lattice";
constexpr int kLaneLabels = 511, kStripLabels = 4095;

struct StripPlan {
    int R;
    size_t lds_bytes, alpha_bytes, acc_bytes, csr_bytes;
    size_t ws_bytes() const { return alpha_bytes + acc_bytes + csr_bytes; }
};

// 512 .. 4095 labels: R states per thread; the workspace is the alpha rows | the sparse sums | the arc lists
StripPlan plan_strip(int batch, int max_frames, int max_labels) {
    StripPlan pl;
    const int S = 2 * max_labels + 1;
    pl.R = 2;
    while (1024 * pl.R < S) pl.R *= 2;
    const size_t NS = (size_t)1024 * pl.R;
    pl.lds_bytes = (2 * (NS + 4) + 2) * sizeof(double);
    pl.alpha_bytes = (size_t)batch * (size_t)max_frames * NS * sizeof(double);
    pl.acc_bytes = (size_t)batch * (NS / 2) * 5 * sizeof(double);
    pl.csr_bytes = (size_t)batch * 2 * NS * sizeof(int32_t);
    return pl;
}

template <int R, bool SPANS, bool WIN>
int launch_strip(const StripParams &p, const StripPlan &pl, int batch, hipStream_t stream) {
    static la::DeviceOnce attr_once;  // once per instantiation, to the planner's budget (pl.lds_bytes never exceeds it)
    auto kern = posterior_strip_kernel<R, SPANS, WIN>;
    if (pl.lds_bytes > 48 * 1024 && attr_once.pending()) {
        LA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
        attr_once.mark();
    }
    la::TimerScope ts("posterior_lattice", stream);
    hipLaunchKernelGGL(kern, dim3(batch), dim3(1024), pl.lds_bytes, stream, p);
    LA_LAUNCH_CHECK();
    return LA_OK;
}

template <bool SPANS, bool WIN>
int launch_strip_face(const StripParams &p, const StripPlan &pl, int batch, hipStream_t stream) {
    switch (pl.R) {
        case 2: return launch_strip<2, SPANS, WIN>(p, pl, batch, stream);
        case 4: return launch_strip<4, SPANS, WIN>(p, pl, batch, stream);
        case 8: return launch_strip<8, SPANS, WIN>(p, pl, batch, stream);
    }
    return LA_EUNSUPPORTED;
}

}  // namespace

extern "C" int la_alignment_posteriors_lattice_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    LA_CHECK_ARG(bytes && batch >= 0 && max_frames > 0 && max_labels > 0, "%s_workspace_bytes: bad arguments", kWho);
    if (max_labels > kStripLabels) {
        la::set_error("%s: max_labels %d exceeds 4095 (8192 lattice states per workgroup)", kWho, max_labels);
        return LA_EUNSUPPORTED;
    }
    if (max_labels <= kLaneLabels) return la_alignment_posteriors_windows_workspace_bytes(batch, max_frames, max_labels, bytes);
    *bytes = plan_strip(batch, max_frames, max_labels).ws_bytes();
    return LA_OK;
}

extern "C" int la_alignment_posteriors_lattice(const float *em, int64_t em_batch_stride, int64_t em_row_stride, const int32_t *labels,
                                               int32_t labels_stride, const int32_t *n_labels, const int32_t *n_frames, int32_t batch,
                                               int32_t max_frames, int32_t max_labels, const int32_t *onset, const int32_t *offset,
                                               int32_t out_stride, int32_t boundary_window, const int32_t *skip_from, int32_t skip_stride,
                                               double skip_penalty, const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride,
                                               float *occupancy, float *onset_prob, float *offset_prob, float *present_prob,
                                               float *span_skip_prob, double *log_z, int32_t *status, float *gamma_out,
                                               int64_t gamma_batch_stride, int64_t gamma_row_stride, void *workspace,
                                               size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (batch == 0) return LA_OK;
    // every argument error is answered here, under this entry's name; the face comes from the pointers that are present
    LA_CHECK_ARG((win_lo == nullptr) == (win_hi == nullptr), "%s: win_lo and win_hi go together (both null: no windows)", kWho);
    const Face face = win_lo ? Face::Windows : skip_from ? Face::Spans : Face::Plain;
    StripParams p{};
    p.set_inputs(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels);
    p.set_spans(skip_from, skip_stride, skip_penalty);
    p.set_windows(win_lo, win_hi, win_stride);
    LA_CHECK_ARG(p.inputs_present(face) && onset && offset, "%s: null input pointer", kWho);
    LA_CHECK_ARG(occupancy && onset_prob && offset_prob && present_prob && span_skip_prob && log_z && status, "%s: null output pointer", kWho);
    LA_CHECK_ARG(p.sizes_ok(batch), "%s: bad sizes", kWho);
    LA_CHECK_ARG(boundary_window >= 0, "%s: negative boundary_window", kWho);
    LA_CHECK_ARG(skip_penalty >= 0.0, "%s: skip_penalty must be >= 0 (and not NaN)", kWho);
    if (max_labels > kStripLabels) {
        la::set_error("%s: max_labels %d exceeds 4095 (8192 lattice states per workgroup)", kWho, max_labels);
        return LA_EUNSUPPORTED;
    }
    // (skip_stride is the row pitch of span_skip_prob whatever the face)
    LA_CHECK_ARG(p.strides_ok(face, out_stride, true) && skip_stride >= max_labels + 1, "%s: strides smaller than max_labels", kWho);
    LA_CHECK_ARG(!gamma_out || (gamma_row_stride >= 2 * (int64_t)max_labels + 1 &&
                                (batch == 1 || gamma_batch_stride >= (int64_t)max_frames * gamma_row_stride)),
                 "%s: gamma strides smaller than [max_frames][2 max_labels + 1]", kWho);
    size_t need = 0;
    const int rc = la_alignment_posteriors_lattice_workspace_bytes(batch, max_frames, max_labels, &need);
    if (rc != LA_OK) return rc;
    LA_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", kWho, workspace_bytes, need);
    LA_CHECK_ARG((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", kWho);

    if (max_labels <= kLaneLabels) {  // the call IS the matching lane-per-state sweep
        if (face == Face::Windows)
            return la_alignment_posteriors_windows(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, batch,
                                                   max_frames, max_labels, onset, offset, out_stride, boundary_window, skip_from, skip_stride,
                                                   skip_penalty, win_lo, win_hi, win_stride, occupancy, onset_prob, offset_prob, present_prob,
                                                   span_skip_prob, log_z, status, gamma_out, gamma_batch_stride, gamma_row_stride, workspace,
                                                   workspace_bytes, stream_);
        if (face == Face::Spans)
            return la_alignment_posteriors_spans(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, batch,
                                                 max_frames, max_labels, onset, offset, out_stride, boundary_window, skip_from, skip_stride,
                                                 skip_penalty, occupancy, onset_prob, offset_prob, present_prob, span_skip_prob, log_z, status,
                                                 gamma_out, gamma_batch_stride, gamma_row_stride, workspace, workspace_bytes, stream_);
        const int st = la_alignment_posteriors(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, batch, max_frames,
                                               max_labels, onset, offset, out_stride, boundary_window, occupancy, onset_prob, offset_prob, log_z,
                                               status, gamma_out, gamma_batch_stride, gamma_row_stride, workspace, workspace_bytes, stream_);
        if (st != LA_OK) return st;
        hipLaunchKernelGGL(no_span_outputs_kernel, dim3(batch), dim3(256), 0, stream, status, n_labels, max_labels, present_prob, out_stride,
                           span_skip_prob, skip_stride);
        LA_LAUNCH_CHECK();
        return LA_OK;
    }

    const StripPlan pl = plan_strip(batch, max_frames, max_labels);
    p.onset = onset, p.offset = offset, p.out_stride = out_stride, p.window = boundary_window;
    p.occupancy = occupancy, p.onset_prob = onset_prob, p.offset_prob = offset_prob;
    p.present_prob = present_prob, p.span_skip_prob = span_skip_prob;
    p.log_z = log_z, p.status = status;
    p.gamma = gamma_out, p.gamma_bs = gamma_batch_stride, p.gamma_rs = gamma_row_stride;
    unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
    p.alpha_ws = reinterpret_cast<double *>(ws);
    p.acc_ws = reinterpret_cast<double *>(ws + pl.alpha_bytes);
    p.csr_ws = reinterpret_cast<int32_t *>(ws + pl.alpha_bytes + pl.acc_bytes);
    switch (face) {
        case Face::Plain: return launch_strip_face<false, false>(p, pl, batch, stream);
        case Face::Spans: return launch_strip_face<true, false>(p, pl, batch, stream);
        case Face::Windows: return launch_strip_face<true, true>(p, pl, batch, stream);
    }
    return LA_EUNSUPPORTED;
}
