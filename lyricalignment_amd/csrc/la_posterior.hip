// la_posterior.hip -- per-character alignment confidence for gfx950: forward-backward (sum-product) on the DP's lattice.
//
// la_viterbi.hip sweeps the lattice of utils/alignment.py:73-119,144-157 max-product and reports ONE path.  The same lattice
// swept sum-product gives the posterior probability gamma_t(k) of every (frame, state) cell under the model, and from it a
// normalised number per character: how much of the model's belief lies inside the reported segment (occupancy) and how much
// of the first-frame / last-frame distribution of the label lies within `boundary_window` frames of the reported onset /
// offset (onset_prob / offset_prob).  The reference has no counterpart (its alignment is max-product only).
//
// Mapping to the hardware (DESIGN.md "Alignment posteriors"): one workgroup per utterance, one lane per lattice state, two
// dependent sweeps of T steps.  Forward: alpha rows to the caller's float64 workspace [batch][max_frames][S_pad].  Backward:
// beta stays in a register; per step every lane forms its gamma, every label lane also its exit term (from the two shifted
// beta_{t+1} values the recurrence fetched anyway) and its entry term (from the stored alpha_{t-1} row one and two states
// down) and adds them to three lane-local sums while t lies inside the label's segment / windows.  No atomics, no second
// pass, one store per label at the end.  S <= 64: ONE wave64, neighbours by DPP wave shifts, no LDS and no barrier in the
// loops.  64 < S <= 1024: up to 16 waves, the previous row through a double-buffered float64 row in LDS, one barrier per
// frame.  Emissions and stored alpha rows are prefetched a block of steps (8; 4 in the multi-wave form) ahead of the dependency chain.
//
// Arithmetic: path scores are float64 (they reach -T * 35).  The log-sum-exp of a step takes its maximum in float64 and the
// correction log(sum exp(x - max)), which lies in [0, ln 3], in float32 (la_lattice.h log_add3, shared with la_loss.hip): <= ~1e-7 absolute per step,
// and a third of the float64 exp / log latency on a kernel that is nothing but a 2T-step latency chain.  Unreachable cells
// are -inf (weight zero); the DP's finite -1e7 is a max-product device and does not appear here.
//
// Optional spans (the SPANS instantiations, la_alignment_posteriors_spans): the lattice of la_viterbi_spans_batch swept sum-product.
// A state at position n with skip_from[n] = a has two more predecessors, J = 2a and (where allowed) J-1, each weighing exp(-penalty).
// Forward mirrors the DP: alpha(J) and alpha(J-1) come from ds_bpermute of the row and of the already-shifted row (one wave) or from
// the LDS row that is exchanged anyway.  Backward is the new part: a state may be the SOURCE of jump arcs into several targets (spans
// may share a start), so the kernel first builds, per source state, the list of its targets in LDS (CSR: out-degree, offset by a
// uniform prefix loop, targets in ascending order; at most 4 arcs per span) and every source lane folds beta_{t+1}(target) - penalty
// over its own list in that fixed order -- no atomics, so a clip's result does not depend on its batch mates.  The trip count is the
// wave's maximum out-degree.  The jump terms are folded with the all-float64 log_add (log_add_jump): the per-step error of log_add3 is unchanged.
// present_prob (sum over t of entry_t(n)) and span_skip_prob (mass of the jump arcs into position n) accumulate on the DESTINATION
// lanes, which hold beta_t and read alpha_{t-1}(J), alpha_{t-1}(J-1) from the stored alpha rows; lanes 2n and 2n+1 are added at the
// end.  "This clip has a span" is a workgroup-uniform test taken once: a span-free clip runs the loops of the plain kernel (its
// present_prob is written as 1: without a jump every path visits every label).
//
// Frame windows (the WIN instantiations, la_alignment_posteriors_windows): the lattice of la_viterbi_windows_batch swept sum-product.  A
// cell (t, s) outside win_lo[s] <= t < win_hi[s] weighs zero.  Each lane keeps its state's lo / hi in two registers and the gate acts on
// the EMISSION, off the loop-carried chain, as in the DP: sum + (double)(-inf) is -inf (sum is never +inf or NaN).  Forward, the block of
// prefetched emissions is gated as it is copied; backward, a step needs the emission twice -- gated in beta_t = sum + e, UNGATED in
// gamma = exp(alpha + beta - e - log_z), where alpha and beta are already -inf outside the window and the gated value would give
// -inf - (-inf) = NaN -- so the gated value is selected beside the ungated one, from the frame index alone.  Entry, exit, present and
// span-skip terms all carry a beta_t or alpha_t factor of the gated cell and need nothing more.  log_z is the windowed one: every output
// is a posterior GIVEN the windows; log_z = -inf (no path inside them) is the existing LA_EINFEASIBLE exit.  WIN exists only together
// with SPANS (a null skip_from = no span anywhere; the once-per-clip has_span test still sends a span-free clip through the plain loops).
#include <type_traits>

#include "la_lattice.h"

namespace {

using namespace la::lattice;

struct PostParams : LatticeIn {
    const int32_t *onset, *offset;
    int32_t out_stride;
    int32_t window;
    float *occupancy, *onset_prob, *offset_prob;
    double *log_z;
    int32_t *status;
    float *present_prob, *span_skip_prob;  // SPANS instantiations only: [batch][out_stride], [batch][skip_stride]
    float *gamma;
    int64_t gamma_bs, gamma_rs;
    double *alpha_ws;  // [batch][max_frames][NT]
};  // (the order of the fields decides how the kernel-argument loads pair up: profiles/lattice_host_refactor.txt section 1)

template <int NW, bool DPP, bool SPANS, bool WIN = false>
__global__ __launch_bounds__(NW * 64) void posterior_kernel(PostParams p) {
    static_assert(!DPP || NW == 1, "DPP neighbour exchange is single-wave only");
    static_assert(!WIN || SPANS, "frame windows are a face of the optional-span forms");
    constexpr int NT = NW * 64;
    // steps per prefetch block: 8; 4 in the multi-wave form, which also prefetches two neighbour alpha columns (1024 threads leave 128
    // VGPRs).  A clip with spans in the multi-wave form prefetches alpha(J) and alpha(J-1) as well, and its steps are several times
    // longer: 2, and 1 at 16 waves (2 spilled 30 VGPRs there, 4 spilled 152)
    constexpr int UP = DPP ? 8 : 4, UJ = DPP ? 8 : (NW == 16 ? 1 : 2);
    // own state at [k + 2]; [0], [1] and [NT + 2], [NT + 3] stay -inf: the neighbours of the first / last states
    __shared__ double rowbuf[DPP ? 1 : 2][DPP ? 1 : NT + 4];
    __shared__ double fin[2];
    // with spans: skip_from row (out-of-range entries -> -1) | out-degree per source state | jump targets per source, CSR (<= 4 arcs per
    // span < 2 NT) | the span mass of every state, for adding lanes 2n and 2n+1
    __shared__ int32_t skip_s[SPANS ? NT / 2 + 1 : 1];
    __shared__ int32_t deg_s[SPANS ? NT : 1];
    __shared__ int32_t tgt_s[SPANS ? 2 * NT : 1];
    __shared__ double pair_s[SPANS ? NT : 1];

    const int b = blockIdx.x;
    const int k = threadIdx.x;
    const int L = p.n_labels[b];
    const int T = p.n_frames[b];
    const int S = 2 * L + 1;
    const int Sg = 2 * p.max_labels + 1;  // <= NT (planned from max_labels)
    const bool odd = (k & 1) != 0;
    const int n = k >> 1;
    const double NEG = -INFINITY;

    float *occ_g = p.occupancy + (int64_t)b * p.out_stride;
    float *onp_g = p.onset_prob + (int64_t)b * p.out_stride;
    float *offp_g = p.offset_prob + (int64_t)b * p.out_stride;
    float *gam = p.gamma ? p.gamma + (int64_t)b * p.gamma_bs : nullptr;
    const bool row_lane = odd && n < p.max_labels;  // the lane that writes label row n (every n < max_labels has one)
    const bool skip_lane = SPANS && !odd && n <= p.max_labels;  // the lane that writes span_skip_prob[n] (end positions 0 .. max_labels)
    float *pres_g = SPANS ? p.present_prob + (int64_t)b * p.out_stride : nullptr;
    float *skp_g = SPANS ? p.span_skip_prob + (int64_t)b * p.skip_stride : nullptr;
    auto zero_gamma_from = [&](int t_from) {
        if (gam && k < Sg)
            for (int t = t_from; t < p.max_frames; ++t) gam[(int64_t)t * p.gamma_rs + k] = 0.f;
    };
    auto fail = [&](int st, double lz) {
        if (row_lane) { occ_g[n] = 0.f; onp_g[n] = 0.f; offp_g[n] = 0.f; }
        if constexpr (SPANS) {
            if (row_lane) pres_g[n] = 0.f;
            if (skip_lane) skp_g[n] = 0.f;
        }
        zero_gamma_from(0);
        if (k == 0) { p.status[b] = st; p.log_z[b] = lz; }
    };
    if (L <= 0) { fail(LA_EEMPTY, 0.0); return; }
    if (T <= 0 || T > p.max_frames || L > p.max_labels) { fail(LA_EINVAL, 0.0); return; }

    const bool valid = k < S;
    const int col = (odd && valid) ? 1 + n : 0;
    const int32_t *lab = p.labels + (int64_t)b * p.labels_stride;
    const bool can_skip = odd && valid && k >= 3 && lab[n] != lab[n - 1];           // k-2 -> k
    const bool can_skip_from = odd && valid && (k + 2 < S) && lab[n + 1] != lab[n];  // k -> k+2
    const float *emb = p.em + (int64_t)b * p.em_bs + col;
    double *aw = p.alpha_ws + (int64_t)b * p.max_frames * NT + k;   // every lane owns a column (k >= S: -inf)

    int parity = 0;
    if (!DPP) {
        if (k < 2) {
            rowbuf[0][k] = NEG; rowbuf[1][k] = NEG;
            rowbuf[0][NT + 2 + k] = NEG; rowbuf[1][NT + 2 + k] = NEG;
        }
    }

    // the span that ends at this state's position n (la_viterbi.hip): J = 2a, the arc from J-1 under the equal-neighbour rule
    int J = -1;
    bool jm1_ok = false;
    if constexpr (SPANS) {
        if (k <= L) {  // (L + 1 <= NT / 2 + 1)
            int a = -1;
            if (!WIN || p.skip_from) a = p.skip_from[(int64_t)b * p.skip_stride + k];   // (windows: a null skip_from = no span anywhere)
            skip_s[k] = (a >= 0 && a < k) ? a : -1;
        }
        __syncthreads();
        if (valid && n >= 1) {
            const int a = skip_s[n];
            if (a >= 0) {
                J = 2 * a;
                jm1_ok = a >= 1 && (!odd || lab[n] != lab[a - 1]);
            }
        }
    }
    // workgroup-uniform, taken once: a clip without a span runs the loops of the plain kernel
    bool has_span = false;
    if constexpr (SPANS) has_span = __syncthreads_or(J >= 0) != 0;
    const double pen = p.penalty;
    const int gather_addr = ((J >= 0 ? J : k) & 63) << 2;  // (single wave: J < S <= 64)
    // jump arcs by SOURCE: state k is J of the spans that start at position (k+1)/2 when even, J-1 of them when odd
    int deg = 0, first = 0, maxdeg = 0;  // out-degree, offset of this lane's list in tgt_s
    if constexpr (SPANS) {
        if (has_span) {
            const int want = (k + 1) >> 1;
            const int mylab = (odd && valid) ? lab[n] : 0;
            auto two = [&](int m) { return m < L && (!odd || lab[m] != mylab); };  // the odd target 2m+1 besides 2m
            if (valid)
                for (int m = want + 1; m <= L; ++m)
                    if (skip_s[m] == want) deg += two(m) ? 2 : 1;
            deg_s[k] = deg;
            __syncthreads();
            for (int i = 0; i < S; ++i) {  // uniform loop, broadcast reads
                const int v = deg_s[i];
                if (i < k) first += v;
            }
            if (valid) {  // ascending: the fold order of the backward sweep
                int i = first;
                for (int m = want + 1; m <= L; ++m) {
                    if (skip_s[m] != want) continue;
                    tgt_s[i++] = 2 * m;
                    if (two(m)) tgt_s[i++] = 2 * m + 1;
                }
            }
            maxdeg = deg;
            for (int o = 32; o; o >>= 1) maxdeg = max(maxdeg, __shfl_xor(maxdeg, o));
            maxdeg = __builtin_amdgcn_readfirstlane(maxdeg);
            __syncthreads();
        }
    }

    // this state's frame window; lanes without a state keep the open one (nothing is read past 2 L_b <= win_stride - 1)
    int wlo = 0, whi = 0x7fffffff;
    if constexpr (WIN) {
        if (valid) {
            wlo = p.win_lo[(int64_t)b * p.win_stride + k];
            whi = p.win_hi[(int64_t)b * p.win_stride + k];
        }
    }
    auto gated = [&](float e, int t) { return (t >= wlo && t < whi) ? e : -INFINITY; };

    // ---- forward: alpha_t(k) = e_t(k) + logsumexp(alpha_{t-1}(k), alpha_{t-1}(k-1), [alpha_{t-1}(k-2)]) ----
    double a = k <= 1 ? (double)(WIN ? gated(emb[0], 0) : emb[0]) : NEG;
    aw[0] = a;
    auto forward = [&](auto has_c) {
        constexpr bool HAS = decltype(has_c)::value;  // this clip has a span
        constexpr int U = HAS ? UJ : UP;
        float ev[U];
        auto fetch = [&](int t0) {
#pragma unroll
            for (int u = 0; u < U; ++u) ev[u] = emb[(int64_t)min(t0 + u, T - 1) * p.em_rs];
        };
        fetch(1);
        for (int t0 = 1; t0 < T; t0 += U) {
            float ec[U];
#pragma unroll
            for (int u = 0; u < U; ++u) ec[u] = WIN ? gated(ev[u], t0 + u) : ev[u];   // the window's gate: off the dependent chain
            if (t0 + U < T) fetch(t0 + U);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u;
                if (t < T) {  // workgroup-uniform
                    double a1, a2, aj = NEG, ajm = NEG;
                    if (DPP) {
                        a1 = wave_shr1(a, NEG);
                        a2 = wave_shr1(a1, NEG);
                        if (HAS) {
                            aj = wave_gather(a, gather_addr);
                            ajm = wave_gather(a1, gather_addr);  // lane J of the shifted row holds alpha(J-1)
                        }
                    } else {
                        double *rb = rowbuf[DPP ? 0 : parity];
                        rb[k + 2] = a;
                        __syncthreads();
                        a1 = rb[k + 1];
                        a2 = rb[k];
                        if (HAS && J >= 0) {
                            aj = rb[J + 2];
                            ajm = rb[J + 1];
                        }
                        parity ^= 1;
                    }
                    if (!can_skip) a2 = NEG;
                    double sum = log_add3(a, a1, a2);
                    if (HAS && J >= 0) sum = log_add_jump(sum, log_add_jump(aj - pen, jm1_ok ? ajm - pen : NEG));
                    a = valid ? sum + (double)ec[u] : NEG;
                    aw[(int64_t)t * NT] = a;
                }
            }
        }
    };
    if (has_span) forward(std::bool_constant<SPANS>{});
    else forward(std::false_type{});
    if (k == S - 1) fin[0] = a;
    if (k == S - 2) fin[1] = a;
    __threadfence_block();   // the backward sweep of the multi-wave form reads alpha columns written by other lanes
    __syncthreads();
    const double log_z = log_add(fin[0], fin[1]);
    if (log_z == -INFINITY) { fail(LA_EINFEASIBLE, log_z); return; }  // no path at all: T too short for the labels

    // ---- backward: beta in a register, gamma / entry / exit per step, lane-local sums ----
    int on = -1, off = -1;
    if (odd && valid) { on = p.onset[(int64_t)b * p.out_stride + n]; off = p.offset[(int64_t)b * p.out_stride + n]; }
    const bool acc_lane = odd && valid && on >= 0 && off > on;
    const int off_last = off - 1, w = p.window;
    double s_occ = 0.0, s_on = 0.0, s_off = 0.0, s_pres = 0.0, s_skip = 0.0;
    double be = NEG;
    auto backward = [&](auto has_c) {
        constexpr bool HAS = decltype(has_c)::value;
        constexpr int U = HAS ? UJ : UP;
        constexpr bool JPF = HAS && !DPP;  // multi-wave form with spans: alpha_{t-1}(J), alpha_{t-1}(J-1) from the workspace as well
        float ev[U];
        double av[U + 1];                 // alpha_t(k) for t = t0 .. t0 - U (the last one is alpha_{t-1} of the block's last step)
        double av1[DPP ? 1 : U], av2[DPP ? 1 : U];  // multi-wave form: alpha_{t-1}(k-1), alpha_{t-1}(k-2) straight from the workspace
        double avj[JPF ? U : 1], avjm[JPF ? U : 1];
        auto fetch = [&](int t0) {  // steps t0, t0 - 1, ..., t0 - U + 1
#pragma unroll
            for (int u = 0; u < U; ++u) ev[u] = emb[(int64_t)max(t0 - u, 0) * p.em_rs];
#pragma unroll
            for (int u = 0; u <= U; ++u) av[u] = aw[(int64_t)max(t0 - u, 0) * NT];
            if (!DPP) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t r = (int64_t)max(t0 - u - 1, 0) * NT;
                    av1[u] = k >= 1 ? aw[r - 1] : NEG;
                    av2[u] = k >= 2 ? aw[r - 2] : NEG;
                    if (JPF) {
                        avj[u] = J >= 0 ? aw[r - k + J] : NEG;
                        avjm[u] = (J >= 0 && jm1_ok) ? aw[r - k + J - 1] : NEG;
                    }
                }
            }
        };
        fetch(T - 1);
        for (int t0 = T - 1; t0 >= 0; t0 -= U) {
            float ec[U];
            double ac[U + 1], ac1[DPP ? 1 : U], ac2[DPP ? 1 : U], acj[JPF ? U : 1], acjm[JPF ? U : 1];
#pragma unroll
            for (int u = 0; u < U; ++u) ec[u] = ev[u];
#pragma unroll
            for (int u = 0; u <= U; ++u) ac[u] = av[u];
            if (!DPP) {
#pragma unroll
                for (int u = 0; u < U; ++u) { ac1[u] = av1[u]; ac2[u] = av2[u]; }
                if (JPF) {
#pragma unroll
                    for (int u = 0; u < U; ++u) { acj[u] = avj[u]; acjm[u] = avjm[u]; }
                }
            }
            if (t0 - U >= 0) fetch(t0 - U);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 - u;
                if (t >= 0) {  // workgroup-uniform
                    const double e = (double)ec[u];
                    // gated in the sums, UNGATED in gamma's subtraction (depends on t and the prefetched value alone: off the chain)
                    const double eg = WIN ? (double)gated(ec[u], t) : e;
                    const double at = ac[u];
                    double out = NEG;  // log weight of leaving state k after frame t: beta_{t+1}(k+1), [beta_{t+1}(k+2)]
                    double js = NEG;   // with spans: the same over the jump arcs that leave state k
                    if (t == T - 1) {
                        be = (k == S - 1 || k == S - 2) ? eg : NEG;
                    } else {
                        double b1, b2;
                        if (DPP) {
                            b1 = wave_shl1(be, NEG);
                            b2 = wave_shl1(b1, NEG);
                        } else {
                            double *rb = rowbuf[DPP ? 0 : parity];
                            rb[k + 2] = be;
                            __syncthreads();
                            b1 = rb[k + 3];
                            b2 = rb[k + 4];
                            parity ^= 1;
                        }
                        if (HAS) {  // fixed order: this lane's targets, ascending
                            const double *rb = rowbuf[DPP ? 0 : parity ^ 1];
                            for (int i = 0; i < maxdeg; ++i) {
                                const bool act = i < deg;
                                const int d = act ? tgt_s[first + i] : k;
                                const double bv = DPP ? wave_gather(be, (d & 63) << 2) : rb[d + 2];
                                if (act) js = log_add_jump(js, bv - pen);
                            }
                        }
                        if (!can_skip_from) b2 = NEG;
                        out = log_add2(b1, b2);
                        double sum = log_add3(be, b1, b2);
                        if (HAS) sum = log_add_jump(sum, js);
                        be = valid ? sum + eg : NEG;
                    }
                    double am1, am2;  // alpha_{t-1}(k-1), alpha_{t-1}(k-2)
                    if (DPP) {
                        am1 = wave_shr1(ac[u + 1], NEG);
                        am2 = wave_shr1(am1, NEG);
                    } else {
                        am1 = ac1[u];
                        am2 = ac2[u];
                    }
                    double jin = NEG;  // with spans: log weight of the jump arcs into state k at frame t (alpha_{t-1} of J, J-1, minus penalty)
                    if (HAS) {
                        double aj, ajm;
                        if (DPP) {
                            aj = wave_gather(ac[u + 1], gather_addr);
                            ajm = wave_gather(am1, gather_addr);
                        } else {
                            aj = acj[JPF ? u : 0];
                            ajm = acjm[JPF ? u : 0];
                        }
                        if (J >= 0 && t > 0) jin = log_add_jump(aj - pen, jm1_ok ? ajm - pen : NEG);
                    }
                    const float g = __expf((float)(at + be - e - log_z));  // alpha and beta both include e_t(k); outside a window both are -inf
                    if (gam && k < Sg) gam[(int64_t)t * p.gamma_rs + k] = g;
                    if (HAS) {
                        if (J >= 0 && t > 0) s_skip += (double)__expf((float)(jin + be - log_z));
                        if (odd && valid) {
                            float en = g;
                            if (t > 0) en = __expf((float)(log_add_jump(log_add2(am1, can_skip ? am2 : NEG), jin) + be - log_z));
                            s_pres += (double)en;
                            if (acc_lane) {
                                if (t >= on && t < off) s_occ += (double)g;
                                if (abs(t - on) <= w) s_on += (double)en;
                                if (abs(t - off_last) <= w) {
                                    const float ex = t == T - 1 ? g : __expf((float)(at + log_add_jump(out, js) - log_z));
                                    s_off += (double)ex;
                                }
                            }
                        }
                    } else if (acc_lane) {
                        if (t >= on && t < off) s_occ += (double)g;
                        if (abs(t - on) <= w) {
                            float en = g;
                            if (t > 0) en = __expf((float)(log_add2(am1, can_skip ? am2 : NEG) + be - log_z));
                            s_on += (double)en;
                        }
                        if (abs(t - off_last) <= w) {
                            const float ex = t == T - 1 ? g : __expf((float)(at + out - log_z));
                            s_off += (double)ex;
                        }
                    }
                }
            }
        }
    };
    if (has_span) backward(std::bool_constant<SPANS>{});
    else backward(std::false_type{});
    if constexpr (SPANS) {
        if (has_span) {
            pair_s[k] = s_skip;
            __syncthreads();
            if (row_lane) pres_g[n] = valid ? (float)s_pres : 0.f;
            if (skip_lane) skp_g[n] = J >= 0 ? (float)(s_skip + pair_s[k + 1]) : 0.f;  // lanes 2n and 2n+1 (0 when n = L)
        } else {  // no jump: every path visits every label
            if (row_lane) pres_g[n] = valid ? 1.f : 0.f;
            if (skip_lane) skp_g[n] = 0.f;
        }
    }
    if (row_lane) {
        occ_g[n] = acc_lane ? (float)(s_occ / (double)(off - on)) : 0.f;
        onp_g[n] = acc_lane ? (float)s_on : 0.f;
        offp_g[n] = acc_lane ? (float)s_off : 0.f;
    }
    zero_gamma_from(T);
    if (k == 0) { p.status[b] = LA_OK; p.log_z[b] = log_z; }
}

// one lane per state; false above 16 waves
bool plan_posterior(int max_labels, int *nw_out) {
    *nw_out = waves_for_labels(max_labels);
    return *nw_out <= 16;
}

template <int NW, bool DPP, bool SPANS, bool WIN>
int launch_posterior(const char *timer, const PostParams &p, int batch, hipStream_t stream) {
    la::TimerScope ts(timer, stream);
    hipLaunchKernelGGL((posterior_kernel<NW, DPP, SPANS, WIN>), dim3(batch), dim3(NW * 64), 0, stream, p);
    LA_LAUNCH_CHECK();
    return LA_OK;
}

template <bool SPANS, bool WIN = false>
int launch_waves(const char *timer, int nw, const PostParams &p, int batch, hipStream_t stream) {
    switch (nw) {
        case 1:
            return la::opts().viterbi_dpp ? launch_posterior<1, true, SPANS, WIN>(timer, p, batch, stream)
                                          : launch_posterior<1, false, SPANS, WIN>(timer, p, batch, stream);
        case 2: return launch_posterior<2, false, SPANS, WIN>(timer, p, batch, stream);
        case 4: return launch_posterior<4, false, SPANS, WIN>(timer, p, batch, stream);
        case 8: return launch_posterior<8, false, SPANS, WIN>(timer, p, batch, stream);
        case 16: return launch_posterior<16, false, SPANS, WIN>(timer, p, batch, stream);
    }
    return LA_EUNSUPPORTED;
}

int query_workspace(Face face, int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    const char *who = face_names(Sweep::Posteriors, face).query;
    LA_CHECK_ARG(bytes && batch >= 0 && max_frames > 0 && max_labels > 0, "%s_workspace_bytes: bad arguments", who);
    int nw;
    if (!plan_posterior(max_labels, &nw)) {
        la::set_error("%s: max_labels %d exceeds 511 (one lane per lattice state, 1024 states per workgroup)", who, max_labels);
        return LA_EUNSUPPORTED;
    }
    *bytes = (size_t)batch * (size_t)max_frames * (size_t)(nw * 64) * sizeof(double);
    return LA_OK;
}

// the arguments the three la_alignment_posteriors* entry points share, by name; the span outputs stay null on the plain face
PostParams shared_params(const float *em, int64_t em_batch_stride, int64_t em_row_stride, const int32_t *labels, int32_t labels_stride,
                         const int32_t *n_labels, const int32_t *n_frames, int32_t max_frames, int32_t max_labels, const int32_t *onset,
                         const int32_t *offset, int32_t out_stride, int32_t boundary_window, float *occupancy, float *onset_prob,
                         float *offset_prob, double *log_z, int32_t *status, float *gamma_out, int64_t gamma_batch_stride,
                         int64_t gamma_row_stride) {
    PostParams p{};
    p.set_inputs(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels);
    p.onset = onset, p.offset = offset, p.out_stride = out_stride, p.window = boundary_window;
    p.occupancy = occupancy, p.onset_prob = onset_prob, p.offset_prob = offset_prob;
    p.log_z = log_z, p.status = status;
    p.gamma = gamma_out, p.gamma_bs = gamma_batch_stride, p.gamma_rs = gamma_row_stride;
    return p;
}

// the three entry points: p holds the caller's arguments (Windows: skip_from may be null, skip_stride stays the row pitch of
// span_skip_prob), the workspace field is set here
int run_posteriors(Face face, PostParams p, int32_t batch, void *workspace, size_t workspace_bytes, hipStream_t stream) {
    const FaceNames &names = face_names(Sweep::Posteriors, face);
    const char *who = names.entry;
    if (batch == 0) return LA_OK;
    LA_CHECK_ARG(p.inputs_present(face) && p.onset && p.offset, "%s: null input pointer", who);
    LA_CHECK_ARG(p.occupancy && p.onset_prob && p.offset_prob && p.log_z && p.status &&
                     (face == Face::Plain || (p.present_prob && p.span_skip_prob)),
                 "%s: null output pointer", who);
    LA_CHECK_ARG(p.sizes_ok(batch), "%s: bad sizes", who);
    LA_CHECK_ARG(p.window >= 0, "%s: negative boundary_window", who);
    LA_CHECK_ARG(p.penalty_ok(face), "%s: skip_penalty must be >= 0 (and not NaN)", who);
    LA_CHECK_ARG(p.strides_ok(face, p.out_stride, true), "%s: strides smaller than max_labels", who);
    LA_CHECK_ARG(!p.gamma || (p.gamma_rs >= 2 * (int64_t)p.max_labels + 1 && (batch == 1 || p.gamma_bs >= (int64_t)p.max_frames * p.gamma_rs)),
                 "%s: gamma strides smaller than [max_frames][2 max_labels + 1]", who);
    int nw;
    if (!plan_posterior(p.max_labels, &nw)) {
        la::set_error("%s: max_labels %d exceeds 511", who, p.max_labels);
        return LA_EUNSUPPORTED;
    }
    const size_t need = (size_t)batch * (size_t)p.max_frames * (size_t)(nw * 64) * sizeof(double);
    LA_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
    LA_CHECK_ARG((uintptr_t)workspace % 8 == 0, "%s: workspace must be 8-byte aligned", who);
    p.alpha_ws = reinterpret_cast<double *>(workspace);
    switch (face) {
        case Face::Plain: return launch_waves<false>(names.timer, nw, p, batch, stream);
        case Face::Spans: return launch_waves<true>(names.timer, nw, p, batch, stream);
        case Face::Windows: return launch_waves<true, true>(names.timer, nw, p, batch, stream);
    }
    return LA_EUNSUPPORTED;
}

}  // namespace

extern "C" int la_alignment_posteriors_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    return query_workspace(Face::Plain, batch, max_frames, max_labels, bytes);
}

extern "C" int la_alignment_posteriors_spans_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    return query_workspace(Face::Spans, batch, max_frames, max_labels, bytes);
}

extern "C" int la_alignment_posteriors_windows_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    return query_workspace(Face::Windows, batch, max_frames, max_labels, bytes);
}

extern "C" int la_alignment_posteriors(const float *em, int64_t em_batch_stride, int64_t em_row_stride, const int32_t *labels,
                                       int32_t labels_stride, const int32_t *n_labels, const int32_t *n_frames, int32_t batch,
                                       int32_t max_frames, int32_t max_labels, const int32_t *onset, const int32_t *offset,
                                       int32_t out_stride, int32_t boundary_window, float *occupancy, float *onset_prob,
                                       float *offset_prob, double *log_z, int32_t *status, float *gamma_out,
                                       int64_t gamma_batch_stride, int64_t gamma_row_stride, void *workspace,
                                       size_t workspace_bytes, void *stream_) {
    PostParams p = shared_params(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels,
                                 onset, offset, out_stride, boundary_window, occupancy, onset_prob, offset_prob, log_z, status,
                                 gamma_out, gamma_batch_stride, gamma_row_stride);
    return run_posteriors(Face::Plain, p, batch, workspace, workspace_bytes, (hipStream_t)stream_);
}

extern "C" int la_alignment_posteriors_spans(const float *em, int64_t em_batch_stride, int64_t em_row_stride, const int32_t *labels,
                                             int32_t labels_stride, const int32_t *n_labels, const int32_t *n_frames, int32_t batch,
                                             int32_t max_frames, int32_t max_labels, const int32_t *onset, const int32_t *offset,
                                             int32_t out_stride, int32_t boundary_window, const int32_t *skip_from, int32_t skip_stride,
                                             double skip_penalty, float *occupancy, float *onset_prob, float *offset_prob,
                                             float *present_prob, float *span_skip_prob, double *log_z, int32_t *status, float *gamma_out,
                                             int64_t gamma_batch_stride, int64_t gamma_row_stride, void *workspace,
                                             size_t workspace_bytes, void *stream_) {
    PostParams p = shared_params(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels,
                                 onset, offset, out_stride, boundary_window, occupancy, onset_prob, offset_prob, log_z, status,
                                 gamma_out, gamma_batch_stride, gamma_row_stride);
    p.set_spans(skip_from, skip_stride, skip_penalty);
    p.present_prob = present_prob, p.span_skip_prob = span_skip_prob;
    return run_posteriors(Face::Spans, p, batch, workspace, workspace_bytes, (hipStream_t)stream_);
}

extern "C" int la_alignment_posteriors_windows(const float *em, int64_t em_batch_stride, int64_t em_row_stride, const int32_t *labels,
                                               int32_t labels_stride, const int32_t *n_labels, const int32_t *n_frames, int32_t batch,
                                               int32_t max_frames, int32_t max_labels, const int32_t *onset, const int32_t *offset,
                                               int32_t out_stride, int32_t boundary_window, const int32_t *skip_from, int32_t skip_stride,
                                               double skip_penalty, const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride,
                                               float *occupancy, float *onset_prob, float *offset_prob, float *present_prob,
                                               float *span_skip_prob, double *log_z, int32_t *status, float *gamma_out,
                                               int64_t gamma_batch_stride, int64_t gamma_row_stride, void *workspace,
                                               size_t workspace_bytes, void *stream_) {
    PostParams p = shared_params(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels,
                                 onset, offset, out_stride, boundary_window, occupancy, onset_prob, offset_prob, log_z, status,
                                 gamma_out, gamma_batch_stride, gamma_row_stride);
    p.set_spans(skip_from, skip_stride, skip_penalty);
    p.set_windows(win_lo, win_hi, win_stride);
    p.present_prob = present_prob, p.span_skip_prob = span_skip_prob;
    return run_posteriors(Face::Windows, p, batch, workspace, workspace_bytes, (hipStream_t)stream_);
}
