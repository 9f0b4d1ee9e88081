// la_posterior.hip -- per-character alignment confidence for gfx950: forward-backward (sum-product) on the DP's lattice, up to 4095 labels.
//
// la_viterbi.hip sweeps the lattice of utils/alignment.py:73-119,144-157 max-product and reports ONE path.  The same lattice
// swept sum-product gives the posterior probability gamma_t(k) of every (frame, state) cell under the model, and from it a
// normalised number per character: how much of the model's belief lies inside the reported segment (occupancy) and how much
// of the first-frame / last-frame distribution of the label lies within `boundary_window` frames of the reported onset /
// offset (onset_prob / offset_prob).  The reference has no counterpart (its alignment is max-product only).
//
// THE CELL (one text: the helpers below, called by both kernels, so a clip gives the same bits in either -- DESIGN.md "Alignment
// posteriors", "Whole-song posteriors").  Two dependent sweeps of T steps.  Forward: alpha_t(k) = e_t(k) + logsumexp(alpha_{t-1}(k),
// (k-1), [(k-2)]), rows to the caller's float64 workspace.  Backward: beta stays in registers; per step every state forms its gamma,
// every label state also its exit term (from the two shifted beta_{t+1} values the recurrence fetched anyway) and its entry term
// (from the stored alpha_{t-1} row one and two states down) and adds them to three sums while t lies inside the label's segment /
// windows.  No atomics, no second pass, one store per label at the end.
//   Arithmetic: path scores are float64 (they reach -T * 35).  The log-sum-exp of a step takes its maximum in float64 and the
// correction log(sum exp(x - max)), which lies in [0, ln 3], in float32 (la_lattice.h log_add3, shared with la_loss.hip): <= ~1e-7
// absolute per step, and a third of the float64 exp / log latency on a kernel that is nothing but a 2T-step latency chain.
// Unreachable cells are -inf (weight zero); the DP's finite -1e7 is a max-product device and does not appear here.
//   Optional spans (SPANS): the lattice of la_viterbi_spans_batch.  A state at position n with skip_from[n] = a has two more
// predecessors, J = 2a and (where allowed) J-1 (la_lattice.h span_source), each weighing exp(-penalty).  Backward a state may be the
// SOURCE of jump arcs into several targets (spans may share a start), so a kernel first builds, per source, the list of its targets
// (CSR: at most 4 arcs per span, ascending target) and every source folds beta_{t+1}(target) - penalty over its own list in that fixed
// order -- no atomics, so a clip's result does not depend on its batch mates.  The jump terms are folded with the all-float64 log_add
// (log_add_jump): the per-step error of log_add3 is unchanged.  present_prob (sum over t of entry_t(n)) and span_skip_prob (mass of
// the jump arcs into position n) accumulate on the DESTINATION states, which hold beta_t and read alpha_{t-1}(J), alpha_{t-1}(J-1)
// from the stored rows; states 2n and 2n+1 are added at the end.  "This clip has a span" is a workgroup-uniform test taken once: a
// span-free clip runs the plain loops (its present_prob is written as 1: without a jump every path visits every label).
//   Frame windows (WIN, only together with SPANS; a null skip_from = no span anywhere): the lattice of la_viterbi_windows_batch.  A
// cell (t, s) outside win_lo[s] <= t < win_hi[s] weighs zero.  The gate acts on the EMISSION, off the loop-carried chain, as in the
// DP: sum + (double)(-inf) is -inf (sum is never +inf or NaN).  Backward a step needs the emission twice -- gated in beta_t = sum + e,
// UNGATED in gamma = exp(alpha + beta - e - log_z), where alpha and beta are already -inf outside the window and the gated value
// would give -inf - (-inf) = NaN -- so the gated value is selected beside the ungated one, from the frame index alone.  Entry, exit,
// present and span-skip terms all carry a beta_t or alpha_t factor of the gated cell and need nothing more.  log_z is the windowed
// one: every output is a posterior GIVEN the windows; log_z = -inf (no path inside them) is the LA_EINFEASIBLE exit.
//
//   Repeatable spans (REP, only on top of SPANS + WIN, null pointers = absent; both layouts): the lattice of
// la_viterbi_repeats_batch.  The odd state 2a+1 with repeat_from[a] = e has two more predecessors, K = 2e and (where allowed) K-1
// (la_lattice.h repeat_source), each weighing exp(-repeat_penalty): the arcs point LEFT, but the sweep is frame-synchronous, so (frame,
// state) stays a DAG.  Forward they are the jump arcs' fetch with the source to the right.  Backward K and K-1 are sources and join the
// per-source arc lists: state k is K of the repeat spans that END at position (k+1)/2 when even, K-1 of them when odd; a list word is
// target | kRepeatArc and so carries its own penalty; FOLD ORDER per source: skip targets ascending, then repeat targets ascending.  A
// path may now visit a label more than once, so entry / exit terms and what is summed from them are EXPECTED COUNTS (include/lyricalign.h
// la_alignment_posteriors_repeats): the repeat-in term joins the entry term (present_prob's slot holds `visits`) and, through js, the exit
// term of its source; repeat_count[a] -- the mass of the repeat arcs into 2a+1 -- accumulates in a register of lane 2a+1, the label's row
// lane.  path_prob[t] = gamma_t(path[t]) is stored by the lane the DP's path names, the path value prefetched with the emissions.  The
// once-per-clip test reads "a span or a repeat arc"; without a repeat arc every shared output has the SPANS + WIN face's bits
// (log_add_jump(x, -inf) is x).  Order per forward cell: the three-term step, J and J-1, K and K-1, the emission last.
//
// LAYOUT 1, up to 511 labels: posterior_kernel<NW, DPP, SPANS, WIN[, REP]>, one workgroup per clip, one lane per state, the sums lane-local
// registers, alpha rows [batch][max_frames][64 NW].  S <= 64: ONE wave64, neighbours by DPP wave shifts, alpha(J) by ds_bpermute, no
// LDS and no barrier in the loops.  64 < S <= 1024: up to 16 waves, the previous row through a double-buffered float64 row in LDS,
// one barrier per frame.  Emissions and stored alpha rows are prefetched a block of steps ahead of the dependency chain.  The arc
// lists live in LDS (out-degree, offset by a uniform prefix loop, targets); the trip count is the wave's maximum out-degree.
//
// LAYOUT 2, 512 .. 4095 labels: posterior_strip_kernel<R, SPANS, WIN[, REP]> on viterbi_strip_kernel's thread layout (la_viterbi.hip): one
// workgroup of 1024 threads per clip, thread tid owns the R CONSECUTIVE states k = tid*R + r (R = 2 / 4 / 8), alpha rows
// [batch][max_frames][1024 R] written as 16-byte pieces.  Neighbours inside a thread are registers; the two rightmost (backward:
// leftmost) states of a thread reach the next thread through a double-buffered float64 row in LDS, one barrier per frame.  Where the
// clip has a span every thread writes all R states into the row and reads alpha(J), alpha(J-1) / its jump targets from the row after
// the barrier, never from the registers the r loop overwrites; backward alpha_{t-1}(J), (J-1) come from the workspace.  What does not
// fit beside two full float64 rows (131,136 B of LDS at R = 8) lives elsewhere:
//   * the arc lists are built once per clip -- skip_from staged in the not-yet-used row buffer, one pass over the end positions for
//     the count and one for the words -- into a per-thread list of (r, target) words in the caller's workspace, ordered by r, then
//     ascending target: folded front to back into js[r] that is the ascending-target order per state.  The first four words stay in
//     registers; the trip count is the wave's maximum list length;
//   * the sparse sums -- occupancy, onset, offset and the span-skip mass -- are read-modify-written by the owning thread in a slot of
//     the workspace behind a divergent branch; present_prob, which every label of a clip with a span adds to at every frame, stays
//     in registers;
//   * states 2n and 2n+1 belong to the same thread (R is even), so span_skip_prob's final add needs no exchange.
//   REP in this layout (la_alignment_posteriors_song): K and km1_ok per owned odd state in registers; forward the K pair comes from the
//   exchanged row like the J pair (a clip with a jump writes all R states there); repeat_from is staged beside skip_from in the
//   not-yet-used row buffer and the repeat arcs join the thread's list behind the skip words of the same state -- ordered by r, then skip
//   targets ascending, then repeat targets ascending: folded front to back that is the documented order per state.  A repeat word is
//   (r << 16) | target | kStripRepeatArc (bit 15: bit 16 belongs to r here, targets are below 8192); at most 2 more arcs per repeat span,
//   one span per start label, so this face's arc area is 3 NS words.  Backward alpha_{t-1}(K), (K-1) come from the workspace rows as
//   (J), (J-1) do; repeat_count[a] accumulates in a sixth workspace slot of the owning thread (AW = 6 for this face only); path_prob[t] is
//   stored by the thread that owns the state the path names, the path value fetched with the emissions.
#include <type_traits>

#include "la_lattice_tile.h"

namespace {

using namespace la::lattice;

struct PostParams : LatticeIn {
    const int32_t *onset, *offset;
    int32_t out_stride;
    int32_t window;
    float *occupancy, *onset_prob, *offset_prob;
    double *log_z;
    int32_t *status;
    float *present_prob, *span_skip_prob;  // [batch][out_stride], [batch][skip_stride]; the plain lane-per-state form writes neither
    float *gamma;
    int64_t gamma_bs, gamma_rs;
    double *alpha_ws;  // [batch][max_frames][states per workgroup]
    // (the order of the fields above decides how the kernel-argument loads pair up: profiles/lattice_host_refactor.txt section 1)
    double *acc_ws;    // strip form: [batch][512 R][5]: occupancy, onset and offset sums of label n, span-skip sums of states 2n and 2n+1
    int32_t *csr_ws;   // strip form: [batch][2048 R]: jump arcs by source thread, (r << 16) | target
};
// what the REP instantiations take besides (every other kernel takes PostParams itself; present_prob is where `visits` goes)
struct RepParams : PostParams {
    const int32_t *repeat_from;  // [batch][repeat_stride], entries 0 .. L_b - 1 of row b are read; null = none
    int32_t repeat_stride;
    double repeat_penalty;
    const int32_t *path;  // [batch][path_stride]: the DP's state per frame; null = not given
    int32_t path_stride;
    float *repeat_count;  // [batch][out_stride]
    float *path_prob;     // [batch][path_stride]; null = not wanted
};
constexpr int kRepeatArc = 1 << 16;  // arc-list word of a repeat arc: its target | this bit (it is charged repeat_penalty)
// the strip form's word is (r << 16) | target, so bit 16 is r's: there a repeat arc sets bit 15, free because a target is below 8192
constexpr int kStripRepeatArc = 1 << 15, kStripTarget = kStripRepeatArc - 1;

// ---- the cell: every expression of the two sweeps that is more than an exchange of neighbours ------------------------------------
// alpha_t(k) before its emission: alpha_{t-1} of k, k-1 and (where the labels differ) k-2
__device__ __forceinline__ double forward_step(double a0, double a1, double a2, bool can_skip) {
    return log_add3(a0, a1, can_skip ? a2 : -INFINITY);
}
// log weight of the jump arcs into a state: alpha of J and (where allowed) J-1, minus the penalty
__device__ __forceinline__ double jump_in(double aj, double ajm, bool jm1_ok, double pen) {
    return log_add_jump(aj - pen, jm1_ok ? ajm - pen : -INFINITY);
}
// beta_t(k) from beta_{t+1} of k, k+1, k+2 (b2 counts where the labels differ), js = the jump arcs that leave k, and the GATED emission;
// out = log weight of leaving state k after frame t
struct BetaStep {
    double be, out;
};
template <bool HAS>
__device__ __forceinline__ BetaStep backward_step(double be, double b1, double b2, bool can_skip_from, double js, double eg, bool valid) {
    if (!can_skip_from) b2 = -INFINITY;
    const double out = log_add2(b1, b2);
    double sum = log_add3(be, b1, b2);
    if (HAS) sum = log_add_jump(sum, js);
    return {valid ? sum + eg : -INFINITY, out};
}
// alpha and beta both include e_t(k), the UNGATED one; outside a window both are -inf
__device__ __forceinline__ float cell_gamma(double at, double be, double e, double log_z) { return __expf((float)(at + be - e - log_z)); }

// What a cell (t, k) adds to the sums of its label / position.  at, be: alpha_t(k), beta_t(k); am1, am2: alpha_{t-1}(k-1), (k-2); jin,
// js: the jump arcs into / out of k (HAS: this clip has a span); label: k is a label state of the clip; acc: and its label has a
// segment; jump_end: a span ends at k.  Entry and exit terms cost an __expf each and are formed only where a sum takes them.
struct Cell {
    double at, be, log_z, am1, am2, jin, out, js;
    float g;
    bool can_skip;
    double rin;  // REP: the repeat arcs into k
};
template <bool HAS, bool REP = false>
__device__ __forceinline__ void add_cell(const Cell &c, bool label, bool acc, bool jump_end, int t, int T, int on, int off, int w,
                                         double &s_occ, double &s_on, double &s_off, double &s_pres, double &s_skip) {
    auto entry = [&] {  // first frame of the label (at t = 0 every path through the cell enters here)
        float en = c.g;
        if (t > 0) {
            double in = log_add2(c.am1, c.can_skip ? c.am2 : -INFINITY);
            if (HAS) in = log_add_jump(in, c.jin);
            if constexpr (REP) {
                if (HAS) in = log_add_jump(in, c.rin);  // a return is an entry of its target (and, through js, an exit of its source)
            }
            en = __expf((float)(in + c.be - c.log_z));
        }
        return en;
    };
    if (HAS && jump_end && t > 0) s_skip += (double)__expf((float)(c.jin + c.be - c.log_z));
    if (HAS ? label : acc) {
        float en = c.g;
        if (HAS) {  // a clip with a span: every label, every frame
            en = entry();
            s_pres += (double)en;
        }
        if (!HAS || acc) {
            if (t >= on && t < off) s_occ += (double)c.g;
            if (abs(t - on) <= w) {
                if (!HAS) en = entry();
                s_on += (double)en;
            }
            if (abs(t - (off - 1)) <= w) {  // last frame of the label
                const float ex = t == T - 1 ? c.g : __expf((float)(c.at + (HAS ? log_add_jump(c.out, c.js) : c.out) - c.log_z));
                s_off += (double)ex;
            }
        }
    }
}

template <int NW, bool DPP, bool SPANS, bool WIN = false, bool REP = false>
__global__ __launch_bounds__(NW * 64) void posterior_kernel(std::conditional_t<REP, RepParams, PostParams> p) {
    static_assert(!DPP || NW == 1, "DPP neighbour exchange is single-wave only");
    static_assert(!WIN || SPANS, "frame windows are a face of the optional-span forms");
    static_assert(!REP || WIN, "repeatable spans are a face of the span + window forms (null pointers: absent)");
    constexpr int NT = NW * 64;
    // steps per prefetch block: 8; 4 in the multi-wave form, which also prefetches two neighbour alpha columns (1024 threads leave 128
    // VGPRs).  A clip with spans in the multi-wave form prefetches alpha(J) and alpha(J-1) as well, and its steps are several times
    // longer: 2, and 1 at 16 waves (2 spilled 30 VGPRs there, 4 spilled 152)
    constexpr int UP = DPP ? 8 : 4, UJ = DPP ? 8 : (NW == 16 ? 1 : 2);
    // own state at [k + 2]; [0], [1] and [NT + 2], [NT + 3] stay -inf: the neighbours of the first / last states
    __shared__ double rowbuf[DPP ? 1 : 2][DPP ? 1 : NT + 4];
    __shared__ double fin[2];
    // with spans: span_first of every end position | out-degree per source state | jump targets per source, CSR (<= 4 arcs per
    // span < 2 NT) | the span mass of every state, for adding lanes 2n and 2n+1
    __shared__ int32_t skip_s[SPANS ? NT / 2 + 1 : 1];
    __shared__ int32_t deg_s[SPANS ? NT : 1];
    // (repeats: at most 2 more arcs per repeat span, one span per start label: < 3 NT in all; and the span end of every start label)
    __shared__ int32_t tgt_s[SPANS ? (REP ? 3 : 2) * NT : 1];
    __shared__ double pair_s[SPANS ? NT : 1];
    __shared__ int32_t rep_s[REP ? NT / 2 : 1];

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
    [[maybe_unused]] auto zero_path_prob_from = [&](int t_from) {
        if constexpr (REP) {
            if (p.path_prob)
                for (int t = t_from + k; t < p.max_frames; t += NT) p.path_prob[(int64_t)b * p.path_stride + t] = 0.f;
        }
    };
    auto fail = [&](int st, double lz) {
        if (row_lane) { occ_g[n] = 0.f; onp_g[n] = 0.f; offp_g[n] = 0.f; }
        if constexpr (SPANS) {
            if (row_lane) pres_g[n] = 0.f;
            if (skip_lane) skp_g[n] = 0.f;
        }
        if constexpr (REP) {
            if (row_lane) p.repeat_count[(int64_t)b * p.out_stride + n] = 0.f;
            zero_path_prob_from(0);
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

    // the span that ends at this state's position n, from the staged row that the arc lists are built from as well
    int J = -1;
    bool jm1_ok = false;
    if constexpr (SPANS) {
        if (k <= L)   // (L + 1 <= NT / 2 + 1; windows: a null skip_from = no span anywhere)
            skip_s[k] = (!WIN || p.skip_from) ? span_first(p.skip_from + (int64_t)b * p.skip_stride, k) : -1;
        __syncthreads();
        const SpanSource src = span_source(skip_s, lab, k, valid);
        J = src.J;
        jm1_ok = src.jm1_ok;
    }
    // the repeat span that starts at this state's label (odd states only); and, for the arc lists, what repeat_source gives every start
    // label a (lane a asks for state 2a+1): K, with kRepeatArc set where K-1 is a source as well, or -1
    [[maybe_unused]] int K = -1;
    [[maybe_unused]] bool km1_ok = false;
    if constexpr (REP) {
        const int32_t *rep_b = p.repeat_from ? p.repeat_from + (int64_t)b * p.repeat_stride : nullptr;
        if (k < L) {  // (L <= NT / 2)
            const RepeatSource of_label = repeat_source(rep_b, lab, 2 * k + 1, true, L);
            rep_s[k] = of_label.K >= 0 ? (of_label.K | (of_label.km1_ok ? kRepeatArc : 0)) : -1;
        }
        const RepeatSource src = repeat_source(rep_b, lab, k, valid, L);
        K = src.K;
        km1_ok = src.km1_ok;
    }
    // workgroup-uniform, taken once: a clip without a span runs the loops of the plain kernel
    // (repeats: neither a span nor a repeat arc; has_span then reads "has a jump of either kind")
    bool has_span = false;
    if constexpr (REP) has_span = __syncthreads_or(J >= 0 || K >= 0) != 0;
    else if constexpr (SPANS) has_span = __syncthreads_or(J >= 0) != 0;
    const double pen = p.penalty;
    const int gather_addr = ((J >= 0 ? J : k) & 63) << 2;  // (single wave: J < S <= 64)
    [[maybe_unused]] double rpen = 0.0;
    if constexpr (REP) rpen = p.repeat_penalty;
    [[maybe_unused]] const int gather_addr_k = ((K >= 0 ? K : k) & 63) << 2;
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
            // repeat arcs: state k is K of the repeat spans that END at position (k+1)/2 when even, K-1 of them when odd (where
            // repeat_source allows that arc); the target is the start label's state 2a+1, to the LEFT of k
            [[maybe_unused]] auto returns_to = [&](int a) {
                const int w = rep_s[a];
                return w >= 0 && (odd ? (w & kRepeatArc) != 0 && (w & (kRepeatArc - 1)) == k + 1 : w == k || w == (k | kRepeatArc));
            };
            if constexpr (REP) {
                if (valid)
                    for (int a = 0; a < want; ++a)
                        if (returns_to(a)) ++deg;
            }
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
                if constexpr (REP) {  // after the skip targets, ascending as well
                    for (int a = 0; a < want; ++a)
                        if (returns_to(a)) tgt_s[i++] = (2 * a + 1) | kRepeatArc;
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
        if (valid && (!REP || p.win_lo)) {  // (repeats: a null window pair = every window open)
            wlo = p.win_lo[(int64_t)b * p.win_stride + k];
            whi = p.win_hi[(int64_t)b * p.win_stride + k];
        }
    }
    auto gated = [&](float e, int t) { return (t >= wlo && t < whi) ? e : -INFINITY; };

    // ---- forward ----
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
                    [[maybe_unused]] double ak = NEG, akm = NEG;
                    if (DPP) {
                        a1 = wave_shr1(a, NEG);
                        a2 = wave_shr1(a1, NEG);
                        if (HAS) {
                            aj = wave_gather(a, gather_addr);
                            ajm = wave_gather(a1, gather_addr);  // lane J of the shifted row holds alpha(J-1)
                            if constexpr (REP) {                   // a source to the right of the target: the same fetch
                                ak = wave_gather(a, gather_addr_k);
                                akm = wave_gather(a1, gather_addr_k);
                            }
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
                        if constexpr (REP) {
                            if (HAS && K >= 0) {
                                ak = rb[K + 2];
                                akm = rb[K + 1];
                            }
                        }
                        parity ^= 1;
                    }
                    double sum = forward_step(a, a1, a2, can_skip);
                    if (HAS && J >= 0) sum = log_add_jump(sum, jump_in(aj, ajm, jm1_ok, pen));
                    if constexpr (REP) {  // after the J terms
                        if (HAS && K >= 0) sum = log_add_jump(sum, jump_in(ak, akm, km1_ok, rpen));
                    }
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

    // ---- backward: beta in a register, lane-local sums ----
    int on = -1, off = -1;
    if (odd && valid) { on = p.onset[(int64_t)b * p.out_stride + n]; off = p.offset[(int64_t)b * p.out_stride + n]; }
    const bool acc_lane = odd && valid && on >= 0 && off > on;
    const int w = p.window;
    double s_occ = 0.0, s_on = 0.0, s_off = 0.0, s_pres = 0.0, s_skip = 0.0;
    [[maybe_unused]] double s_rep = 0.0;  // lane 2a+1: the mass of the repeat arcs into it
    [[maybe_unused]] const int32_t *path_b = nullptr;
    [[maybe_unused]] float *pp_g = nullptr;
    if constexpr (REP) {
        if (p.path_prob) {  // (the host: only with a path)
            path_b = p.path + (int64_t)b * p.path_stride;
            pp_g = p.path_prob + (int64_t)b * p.path_stride;
        }
    }
    double be = NEG;
    auto backward = [&](auto has_c) {
        constexpr bool HAS = decltype(has_c)::value;
        constexpr int U = HAS ? UJ : UP;
        // multi-wave form with spans: alpha_{t-1}(J), alpha_{t-1}(J-1) from the workspace as well (not in the 16-wave repeat form: below)
        constexpr bool JPF = HAS && !DPP && !(REP && NW == 16);
        float ev[U];
        double av[U + 1];                 // alpha_t(k) for t = t0 .. t0 - U (the last one is alpha_{t-1} of the block's last step)
        double av1[DPP ? 1 : U], av2[DPP ? 1 : U];  // multi-wave form: alpha_{t-1}(k-1), alpha_{t-1}(k-2) straight from the workspace
        double avj[JPF ? U : 1], avjm[JPF ? U : 1];
        // and alpha_{t-1}(K), alpha_{t-1}(K-1) -- except at 16 waves, where the registers do not hold them a block ahead (they feed the
        // sums alone, not beta: the load at the step's start is off the loop-carried chain)
        constexpr bool KPF = JPF && REP && NW != 16;
        [[maybe_unused]] double avk[KPF ? U : 1], avkm[KPF ? U : 1];
        [[maybe_unused]] int pv[REP ? U : 1];  // the reported path's state at the block's frames (workgroup-uniform)
        auto fetch = [&](int t0) {  // steps t0, t0 - 1, ..., t0 - U + 1
            if constexpr (REP) {
#pragma unroll
                for (int u = 0; u < U; ++u) pv[u] = path_b ? path_b[max(t0 - u, 0)] : -1;
            }
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
                    if constexpr (KPF) {
                        avk[u] = K >= 0 ? aw[r - k + K] : NEG;
                        avkm[u] = (K >= 0 && km1_ok) ? aw[r - k + K - 1] : NEG;
                    }
                }
            }
        };
        fetch(T - 1);
        for (int t0 = T - 1; t0 >= 0; t0 -= U) {
            float ec[U];
            double ac[U + 1], ac1[DPP ? 1 : U], ac2[DPP ? 1 : U], acj[JPF ? U : 1], acjm[JPF ? U : 1];
            [[maybe_unused]] double ack[KPF ? U : 1], ackm[KPF ? U : 1];
            [[maybe_unused]] int pc[REP ? U : 1];
            if constexpr (REP) {
#pragma unroll
                for (int u = 0; u < U; ++u) pc[u] = pv[u];
            }
            if constexpr (KPF) {
#pragma unroll
                for (int u = 0; u < U; ++u) { ack[u] = avk[u]; ackm[u] = avkm[u]; }
            }
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
                    Cell c;
                    c.at = ac[u], c.log_z = log_z, c.can_skip = can_skip;
                    c.out = NEG, c.js = NEG, c.jin = NEG, c.rin = NEG;
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
                        if (HAS) {  // fixed order: this lane's targets, ascending (repeats: skip targets, then repeat targets)
                            const double *rb = rowbuf[DPP ? 0 : parity ^ 1];
                            for (int i = 0; i < maxdeg; ++i) {
                                const bool act = i < deg;
                                if constexpr (REP) {  // every arc carries its own penalty
                                    const int ent = act ? tgt_s[first + i] : k;
                                    const int d = ent & (kRepeatArc - 1);
                                    const double bv = DPP ? wave_gather(be, (d & 63) << 2) : rb[d + 2];
                                    if (act) c.js = log_add_jump(c.js, bv - ((ent & kRepeatArc) ? rpen : pen));
                                } else {
                                    const int d = act ? tgt_s[first + i] : k;
                                    const double bv = DPP ? wave_gather(be, (d & 63) << 2) : rb[d + 2];
                                    if (act) c.js = log_add_jump(c.js, bv - pen);
                                }
                            }
                        }
                        const BetaStep st = backward_step<HAS>(be, b1, b2, can_skip_from, c.js, eg, valid);
                        be = st.be, c.out = st.out;
                    }
                    if (DPP) {
                        c.am1 = wave_shr1(ac[u + 1], NEG);
                        c.am2 = wave_shr1(c.am1, NEG);
                    } else {
                        c.am1 = ac1[u];
                        c.am2 = ac2[u];
                    }
                    if (HAS) {
                        double aj, ajm;
                        if (DPP) {
                            aj = wave_gather(ac[u + 1], gather_addr);
                            ajm = wave_gather(c.am1, gather_addr);
                        } else if (JPF) {
                            aj = acj[JPF ? u : 0];
                            ajm = acjm[JPF ? u : 0];
                        } else {  // the 16-wave repeat form: read at the step's start (they feed the sums alone, not beta)
                            const double *prow = aw + (int64_t)max(t - 1, 0) * NT - k;
                            aj = J >= 0 ? prow[J] : NEG;
                            ajm = (J >= 0 && jm1_ok) ? prow[J - 1] : NEG;
                        }
                        if (J >= 0 && t > 0) c.jin = jump_in(aj, ajm, jm1_ok, pen);
                        if constexpr (REP) {
                            double ak, akm;
                            if (DPP) {
                                ak = wave_gather(ac[u + 1], gather_addr_k);
                                akm = wave_gather(c.am1, gather_addr_k);
                            } else if (KPF) {
                                ak = ack[KPF ? u : 0];
                                akm = ackm[KPF ? u : 0];
                            } else {
                                const double *prow = aw + (int64_t)max(t - 1, 0) * NT - k;
                                ak = K >= 0 ? prow[K] : NEG;
                                akm = (K >= 0 && km1_ok) ? prow[K - 1] : NEG;
                            }
                            if (K >= 0 && t > 0) c.rin = jump_in(ak, akm, km1_ok, rpen);
                        }
                    }
                    c.be = be;
                    c.g = cell_gamma(c.at, be, e, log_z);
                    if (gam && k < Sg) gam[(int64_t)t * p.gamma_rs + k] = c.g;
                    if constexpr (REP) {
                        // gamma at the reported path: stored by the lane whose state the path names (a value that names none: 0, by lane 0)
                        const bool named = pc[u] >= 0 && pc[u] < S;
                        if (pp_g && k == (named ? pc[u] : 0)) pp_g[t] = named ? c.g : 0.f;
                        if (HAS && K >= 0 && t > 0) s_rep += (double)__expf((float)(c.rin + be - log_z));
                    }
                    add_cell<HAS, REP>(c, odd && valid, acc_lane, J >= 0, t, T, on, off, w, s_occ, s_on, s_off, s_pres, s_skip);
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
    if constexpr (REP) {
        if (row_lane) p.repeat_count[(int64_t)b * p.out_stride + n] = (has_span && valid) ? (float)s_rep : 0.f;
        zero_path_prob_from(T);
    }
    zero_gamma_from(T);
    if (k == 0) { p.status[b] = LA_OK; p.log_z[b] = log_z; }
}

template <int R, bool SPANS, bool WIN, bool REP = false>
__global__ __launch_bounds__(1024) void posterior_strip_kernel(std::conditional_t<REP, RepParams, PostParams> p) {
    static_assert(!WIN || SPANS, "frame windows are a face of the optional-span forms");
    static_assert(!REP || WIN, "repeatable spans are a face of the span + window forms (null pointers: absent)");
    static_assert(R == 2 || R == 4 || R == 8, "states per thread");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NT = 1024, NS = NT * R, NL = R / 2, ROW = NS + 4;
    // frames per prefetch block (emissions, and backward the alpha rows): the span-free loops / the loops of a clip with a span
    constexpr int UP = R == 2 ? 4 : R == 4 ? 2 : 1, UJ = 1;
    constexpr int CR = 4;  // arc words kept in registers
    constexpr int AW = REP ? 6 : 5;  // sums per label kept in the workspace (repeats: and the mass of the repeat arcs into the label)
    constexpr int CW = REP ? 3 : 2;  // arc words per state in the workspace (repeats: at most 2 more arcs per span, one span per start label)
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
    [[maybe_unused]] auto zero_path_prob_from = [&](int t_from) {
        if constexpr (REP) {
            if (p.path_prob)
                for (int t = t_from + tid; t < p.max_frames; t += NT) p.path_prob[(int64_t)b * p.path_stride + t] = 0.f;
        }
    };
    auto fail = [&](int st, double lz) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int n = n0 + i;
            if (n < p.max_labels) { occ_g[n] = 0.f; onp_g[n] = 0.f; offp_g[n] = 0.f; pres_g[n] = 0.f; }
            if (n <= p.max_labels) skp_g[n] = 0.f;
            if constexpr (REP) {
                if (n < p.max_labels) p.repeat_count[(int64_t)b * p.out_stride + n] = 0.f;
            }
        }
        if constexpr (REP) zero_path_prob_from(0);
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

    // the span that ends at each owned state's position, and each owned state's frame window
    [[maybe_unused]] const int32_t *skip_b = nullptr;
    [[maybe_unused]] int J[SPANS ? R : 1];
    [[maybe_unused]] bool jm1_ok[SPANS ? R : 1];
    [[maybe_unused]] int wlo[WIN ? R : 1], whi[WIN ? R : 1];
    // the repeat span that starts at each owned ODD state's label (k0 is even: the odd states are r = 2 i + 1)
    [[maybe_unused]] const int32_t *rep_b = nullptr;
    [[maybe_unused]] int K[REP ? NL : 1];
    [[maybe_unused]] bool km1_ok[REP ? NL : 1];
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
        if constexpr (REP) {
            if (p.repeat_from) rep_b = p.repeat_from + (int64_t)b * p.repeat_stride;
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const RepeatSource src = repeat_source(rep_b, lab, k0 + 2 * i + 1, k0 + 2 * i + 1 < S, L);
                K[i] = src.K;
                km1_ok[i] = src.km1_ok;
                any |= src.K >= 0;
            }
        }
        // workgroup-uniform, taken once: a clip without a span (repeats: without a jump of either kind) runs the plain loops
        has_span = __syncthreads_or(any) != 0;
    }
    if constexpr (WIN) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            wlo[r] = 0, whi[r] = 0x7fffffff;
            if (k0 + r < S && (!REP || p.win_lo)) {  // (repeats: a null window pair = every window open)
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
    [[maybe_unused]] double rpen = 0.0;
    if constexpr (REP) rpen = p.repeat_penalty;

    // jump arcs by SOURCE: state k is J of the spans that start at position (k+1)/2 when even, J-1 of them when odd.  This thread's
    // list: tdeg words from csr[0], ordered by r, then ascending target (repeats: per r the skip targets, then the repeat targets)
    int tdeg = 0, maxdeg = 0;
    [[maybe_unused]] int ent_reg[CR] = {0, 0, 0, 0};
    [[maybe_unused]] const int32_t *csr = nullptr;
    if constexpr (SPANS) {
        if (has_span) {
            int32_t *skip_s = reinterpret_cast<int32_t *>(rowbuf);      // [L + 1] <= 4 NS bytes
            int32_t *tot_s = reinterpret_cast<int32_t *>(rowbuf + ROW);  // [NT]
            // repeats: beside it, what repeat_source gives every start label a: K, with kStripRepeatArc set where K-1 is a source as
            // well, or -1 ([L] <= NS / 2 - 1 words behind the NS / 2 of skip_s: 4 NS bytes in all)
            [[maybe_unused]] int32_t *rep_s = skip_s + NS / 2;
            if constexpr (REP) {
                for (int m = tid; m <= L; m += NT) skip_s[m] = skip_b ? span_first(skip_b, m) : -1;
                for (int a = tid; a < L; a += NT) {
                    const RepeatSource of_label = repeat_source(rep_b, lab, 2 * a + 1, true, L);
                    rep_s[a] = of_label.K >= 0 ? (of_label.K | (of_label.km1_ok ? kStripRepeatArc : 0)) : -1;
                }
            } else {
                for (int m = tid; m <= L; m += NT) skip_s[m] = span_first(skip_b, m);
            }
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
            // repeat arcs: state k is K of the repeat spans that END at position (k+1)/2 when even, K-1 of them when odd (where
            // repeat_source allows that arc); the target is the start label's state 2a+1, to the LEFT of k.  One pass over the start labels
            [[maybe_unused]] auto returns = [&](auto emit) {
                const int a_end = min(L, n0 + NL);
                for (int a = 0; a < a_end; ++a) {
                    const int w = rep_s[a];
                    if (w < 0) continue;
                    const int e = (w & kStripTarget) >> 1;
                    if (e < n0 || e > n0 + NL) continue;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if (((k0 + r + 1) >> 1) != e) continue;
                        if (!(r & 1) || (w & kStripRepeatArc)) emit(r, (2 * a + 1) | kStripRepeatArc);
                    }
                }
            };
            int cnt[R];
#pragma unroll
            for (int r = 0; r < R; ++r) cnt[r] = 0;
            arcs([&](int r, int) { ++cnt[r]; });
            if constexpr (REP) returns([&](int r, int) { ++cnt[r]; });
#pragma unroll
            for (int r = 0; r < R; ++r) tdeg += cnt[r];
            tot_s[tid] = tdeg;
            __syncthreads();
            int first = 0;
            for (int i = 0; i < NT; ++i) {  // uniform loop, broadcast reads
                const int v = tot_s[i];
                if (i < tid) first += v;
            }
            int32_t *mine = p.csr_ws + (int64_t)b * (CW * NS) + first;  // at most 4 arcs per span: < 2 NS in all (repeats: < 3 NS)
            int pos[R];                                                 // where the list of state r goes on: by r, then ascending target
            pos[0] = 0;
#pragma unroll
            for (int r = 1; r < R; ++r) pos[r] = pos[r - 1] + cnt[r - 1];
            arcs([&](int r, int d) { mine[pos[r]++] = (r << 16) | d; });
            // behind the skip targets of the same state: pos[r] has gone past them (cnt[r] counted both kinds)
            if constexpr (REP) returns([&](int r, int d) { mine[pos[r]++] = (r << 16) | d; });
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

    // ---- forward ----
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
                        double sum = forward_step(prev[r + 2], prev[r + 1], prev[r], can_skip[r]);
                        if constexpr (HAS) {
                            if (J[r] >= 0) sum = log_add_jump(sum, jump_in(rb[J[r] + 2], rb[J[r] + 1], jm1_ok[r], pen));  // from the row, never from a[]
                            if constexpr (REP) {  // after the J terms; the source lies to the right, in the same row
                                if ((r & 1) && K[r >> 1] >= 0)
                                    sum = log_add_jump(sum, jump_in(rb[K[r >> 1] + 2], rb[K[r >> 1] + 1], km1_ok[r >> 1], rpen));
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

    // ---- backward: beta in registers, the sparse sums in the workspace ----
    int on[NL], off[NL];
    bool acc_lane[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        on[i] = -1, off[i] = -1;
        if (k0 + 2 * i + 1 < S) { on[i] = p.onset[(int64_t)b * p.out_stride + n0 + i]; off[i] = p.offset[(int64_t)b * p.out_stride + n0 + i]; }
        acc_lane[i] = on[i] >= 0 && off[i] > on[i];
    }
    const int w = p.window;
    [[maybe_unused]] const int32_t *path_b = nullptr;
    [[maybe_unused]] float *pp_g = nullptr;
    if constexpr (REP) {
        if (p.path_prob) {  // (the host: only with a path)
            path_b = p.path + (int64_t)b * p.path_stride;
            pp_g = p.path_prob + (int64_t)b * p.path_stride;
        }
    }
    auto backward = [&](auto has_c) {
        constexpr bool HAS = decltype(has_c)::value;
        constexpr int U = HAS ? UJ : UP;
        // the next block's emissions and alpha rows are fetched while this block is computed, except where the clip has a span and
        // a thread owns 4 or 8 states: there the loads of a frame are issued at its start (the registers do not hold two generations)
        constexpr bool PF = !HAS || R == 2;
        double s_pres[NL];  // (span-free clip: never added to)
#pragma unroll
        for (int i = 0; i < NL; ++i) s_pres[i] = 0.0;
        double be[R];
#pragma unroll
        for (int r = 0; r < R; ++r) be[r] = NEG;
        // alpha rows: `top` is alpha_t0 of the next block (carried, not fetched twice); nx[u] is row t0 - 1 - u, nl[u] the two values left of it
        double top[R], nx[U][R], nl[U][2];
        float ev[U][NL + 1];
        [[maybe_unused]] int pv[REP ? U : 1];  // the reported path's state at the block's frames (workgroup-uniform)
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
            if constexpr (REP) {
#pragma unroll
                for (int u = 0; u < U; ++u) pv[u] = path_b ? path_b[max(t0 - u, 0)] : -1;
            }
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
            [[maybe_unused]] int pc[REP ? U : 1];
            if constexpr (REP) {
#pragma unroll
                for (int u = 0; u < U; ++u) pc[u] = pv[u];
            }
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
                                const int d = act ? (ent & (REP ? kStripTarget : 0xffff)) : k0, er = ent >> 16;
                                const double bv = rb[d + 2];
                                double cur = js[0];
#pragma unroll
                                for (int r = 1; r < R; ++r) cur = er == r ? js[r] : cur;
                                double apen = pen;  // repeats: every arc carries its own penalty
                                if constexpr (REP) apen = (ent & kStripRepeatArc) ? rpen : pen;
                                const double res = log_add_jump(cur, bv - apen);
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
                        const int k = k0 + r, i = r >> 1;
                        const bool odd = (r & 1) != 0, valid = k < S;
                        const float ef = odd ? ec[u][1 + i] : ec[u][0];
                        const double e = (double)ef;
                        // gated in the sums, UNGATED in gamma's subtraction (depends on t and the prefetched value alone: off the chain)
                        const double eg = (double)gated(ef, t, r);
                        const double at = ar[u][r];
                        double out = NEG;  // log weight of leaving state k after frame t
                        if (t == T - 1) {
                            be[r] = (k == S - 1 || k == S - 2) ? eg : NEG;
                            if constexpr (HAS) js[r] = NEG;
                        } else {
                            double jr = NEG;
                            if constexpr (HAS) jr = js[r];
                            const BetaStep st = backward_step<HAS>(nb[r], nb[r + 1], nb[r + 2], can_skip_from[r], jr, eg, valid);
                            be[r] = st.be, out = st.out;
                        }
                        // alpha_{t-1}(k-1), alpha_{t-1}(k-2)
                        const double am1 = r >= 1 ? ar[u + 1][r >= 1 ? r - 1 : 0] : al[u][0];
                        const double am2 = r >= 2 ? ar[u + 1][r >= 2 ? r - 2 : 0] : al[u][r == 0 ? 1 : 0];
                        [[maybe_unused]] double jin = NEG;  // with spans: log weight of the jump arcs into state k at frame t
                        if constexpr (HAS) {
                            if (J[r] >= 0 && t > 0) {
                                const double *prow = aw + (int64_t)(t - 1) * NS;
                                jin = jump_in(prow[J[r]], jm1_ok[r] ? prow[J[r] - 1] : NEG, jm1_ok[r], pen);
                            }
                        }
                        const float g = cell_gamma(at, be[r], e, log_z);
                        if (gam && k < Sg) gam[(int64_t)t * p.gamma_rs + k] = g;
                        [[maybe_unused]] double rin = NEG;  // repeats: log weight of the repeat arcs into state k at frame t
                        if constexpr (REP) {
                            // gamma at the reported path: stored by the thread that owns the state the path names (a value that names none: 0,
                            // by state 0's)
                            const bool named = pc[u] >= 0 && pc[u] < S;
                            if (pp_g && k == (named ? pc[u] : 0)) pp_g[t] = named ? g : 0.f;
                            if constexpr (HAS) {
                                if (odd && K[i] >= 0 && t > 0) {
                                    const double *prow = aw + (int64_t)(t - 1) * NS;
                                    rin = jump_in(prow[K[i]], km1_ok[i] ? prow[K[i] - 1] : NEG, km1_ok[i], rpen);
                                    acc[AW * i + 5] += (double)__expf((float)(rin + be[r] - log_z));
                                }
                            }
                        }
                        if constexpr (HAS) {
                            // add_cell<true>'s text, kept here: through the helper the 8-states-per-thread span faces (which spill
                            // 140 / 182 VGPRs) came out 3 % slower on the anchors + optional lines leg (profiles/posterior_refactor.txt)
                            if (J[r] >= 0 && t > 0) acc[AW * i + 3 + (r & 1)] += (double)__expf((float)(jin + be[r] - log_z));
                            if (odd && valid) {
                                float en = g;
                                if constexpr (REP) {  // a return is an entry of its target (and, through js, an exit of its source)
                                    if (t > 0)
                                        en = __expf((float)(log_add_jump(log_add_jump(log_add2(am1, can_skip[r] ? am2 : NEG), jin), rin) + be[r] - log_z));
                                } else {
                                    if (t > 0) en = __expf((float)(log_add_jump(log_add2(am1, can_skip[r] ? am2 : NEG), jin) + be[r] - log_z));
                                }
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
                        } else {
                            add_cell<false>(Cell{at, be[r], log_z, am1, am2, NEG, out, NEG, g, can_skip[r]}, odd && valid, odd && acc_lane[i], false, t,
                                            T, on[i], off[i], w, acc[AW * i], acc[AW * i + 1], acc[AW * i + 2], s_pres[i], acc[AW * i + 3]);
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
                if constexpr (REP) {
                    if (n < p.max_labels) p.repeat_count[(int64_t)b * p.out_stride + n] = valid ? (float)acc[AW * i + 5] : 0.f;
                }
            } else {  // no jump: every path visits every label
                if (n < p.max_labels) pres_g[n] = valid ? 1.f : 0.f;
                if (n <= p.max_labels) skp_g[n] = 0.f;
                if constexpr (REP) {
                    if (n < p.max_labels) p.repeat_count[(int64_t)b * p.out_stride + n] = 0.f;
                }
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
    if constexpr (REP) zero_path_prob_from(T);
    zero_gamma_from(T);
    if (tid == 0) { p.status[b] = LA_OK; p.log_z[b] = log_z; }
}

// the lattice entry on the plain lane-per-state form, which wrote the five common outputs: the span outputs of a lattice without a
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

// ---- host ----
// up to 511 labels: nw waves, one lane per state, the workspace is the alpha rows.  512 .. 4095: R states per thread, the workspace is
// the alpha rows | the sparse sums | the arc lists, the two rows in dynamic LDS.  rep (the song entry): the strip form's REP face, with
// 6 sums per label instead of 5 and 3 arc words per state instead of 2 (at most 4 arcs per optional span, at most 2 per repeat span)
struct PostPlan {
    int nw, R;
    size_t lds_bytes, alpha_bytes, acc_bytes, csr_bytes;
    size_t ws_bytes() const { return alpha_bytes + acc_bytes + csr_bytes; }
};

bool plan_posterior(int batch, int max_frames, int max_labels, int label_limit, PostPlan *pl, bool rep = false) {
    Tile tile;
    if (!plan_tile(max_labels, label_limit, &tile)) return false;
    *pl = PostPlan{};
    pl->nw = tile.nw;
    pl->R = tile.r > 1 ? tile.r : 0;   // (0: one lane per state)
    const size_t NS = pl->R ? (size_t)1024 * pl->R : (size_t)pl->nw * 64;
    pl->alpha_bytes = (size_t)batch * (size_t)max_frames * NS * sizeof(double);
    if (pl->R) {
        pl->lds_bytes = (2 * (NS + 4) + 2) * sizeof(double);
        pl->acc_bytes = (size_t)batch * (NS / 2) * (rep ? 6 : 5) * sizeof(double);
        pl->csr_bytes = (size_t)batch * (rep ? 3 : 2) * NS * sizeof(int32_t);
    }
    return true;
}

template <bool SPANS, bool WIN>
int launch_face(const char *timer, const PostParams &p, const PostPlan &pl, int batch, hipStream_t stream) {
    switch (pl.R) {
        case 2: return launch<posterior_strip_kernel<2, SPANS, WIN>>(timer, 1024, p, pl, batch, stream);
        case 4: return launch<posterior_strip_kernel<4, SPANS, WIN>>(timer, 1024, p, pl, batch, stream);
        case 8: return launch<posterior_strip_kernel<8, SPANS, WIN>>(timer, 1024, p, pl, batch, stream);
    }
    switch (pl.nw) {
        case 1:
            if (la::opts().viterbi_dpp) return launch<posterior_kernel<1, true, SPANS, WIN>>(timer, 64, p, pl, batch, stream);
            return launch<posterior_kernel<1, false, SPANS, WIN>>(timer, 64, p, pl, batch, stream);
        case 2: return launch<posterior_kernel<2, false, SPANS, WIN>>(timer, 128, p, pl, batch, stream);
        case 4: return launch<posterior_kernel<4, false, SPANS, WIN>>(timer, 256, p, pl, batch, stream);
        case 8: return launch<posterior_kernel<8, false, SPANS, WIN>>(timer, 512, p, pl, batch, stream);
        case 16: return launch<posterior_kernel<16, false, SPANS, WIN>>(timer, 1024, p, pl, batch, stream);
    }
    return LA_EUNSUPPORTED;
}

// the repeat face sits on top of the span + window one whatever is given: null pointers are "absent" inside the kernel
int launch_repeats(const char *timer, const RepParams &p, const PostPlan &pl, int batch, hipStream_t stream) {
    // static LDS of the widest form: two rows, fin, skip_s, deg_s, tgt_s (3 NT words with the repeat arcs), pair_s, rep_s
    static_assert((2 * (1024 + 4) + 2 + 1024) * sizeof(double) + (1024 / 2 + 1 + 1024 + 3 * 1024 + 1024 / 2) * sizeof(int32_t) <= 64 * 1024 &&
                      64 * 1024 <= kLdsBudget, "the arc lists with the repeat arcs fit the workgroup's LDS");
    switch (pl.R) {
        case 2: return launch<posterior_strip_kernel<2, true, true, true>, RepParams>(timer, 1024, p, pl, batch, stream);
        case 4: return launch<posterior_strip_kernel<4, true, true, true>, RepParams>(timer, 1024, p, pl, batch, stream);
        case 8: return launch<posterior_strip_kernel<8, true, true, true>, RepParams>(timer, 1024, p, pl, batch, stream);
    }
    switch (pl.nw) {
        case 1:
            if (la::opts().viterbi_dpp) return launch<posterior_kernel<1, true, true, true, true>, RepParams>(timer, 64, p, pl, batch, stream);
            return launch<posterior_kernel<1, false, true, true, true>, RepParams>(timer, 64, p, pl, batch, stream);
        case 2: return launch<posterior_kernel<2, false, true, true, true>, RepParams>(timer, 128, p, pl, batch, stream);
        case 4: return launch<posterior_kernel<4, false, true, true, true>, RepParams>(timer, 256, p, pl, batch, stream);
        case 8: return launch<posterior_kernel<8, false, true, true, true>, RepParams>(timer, 512, p, pl, batch, stream);
        case 16: return launch<posterior_kernel<16, false, true, true, true>, RepParams>(timer, 1024, p, pl, batch, stream);
    }
    return LA_EUNSUPPORTED;
}

// What the six entries (and their workspace queries) differ in.  la_alignment_posteriors_lattice takes its face from the pointers that
// are present, always writes the span outputs (so skip_stride is their row pitch whatever the face) and reports its label limit before
// the strides; up to 511 labels its call then IS the matching entry's sweep, under that entry's timer.
struct Entry {
    FaceNames names;
    int label_limit;
    size_t ws_align;      // the strip kernel moves alpha rows as 16-byte pieces
    bool span_outputs;    // present_prob and span_skip_prob are required
    bool limit_first;     // the label limit is reported before the stride checks (the other entries: after them)
    bool repeats;         // takes the RepParams part (the REP faces)
    const char *over_entry, *over_query;   // the label-limit message of the entry and of its workspace query
};
enum EntryId { kPlain, kSpans, kWindows, kLattice, kRepeats, kSong };   // the first three are (int)Face of the entry's fixed face; the others: decided per call
static_assert(kPlain == (int)Face::Plain && kSpans == (int)Face::Spans && kWindows == (int)Face::Windows, "kEntries rows follow Face");
constexpr char kOverLanes[] = "%s: max_labels %d exceeds 511", kOverStrip[] = "%s: max_labels %d exceeds 4095 (8192 lattice states per workgroup)";
constexpr char kOverLanesQuery[] = "%s: max_labels %d exceeds 511 (one lane per lattice state, 1024 states per workgroup)";
// (la_alignment_posteriors_song is la_alignment_posteriors_repeats without the 511-label limit: up to 511 labels its call IS that
// entry's sweep, under that entry's timer)
const Entry kEntries[6] = {
    {face_names(Sweep::Posteriors, Face::Plain), 511, 8, false, false, false, kOverLanes, kOverLanesQuery},
    {face_names(Sweep::Posteriors, Face::Spans), 511, 8, true, false, false, kOverLanes, kOverLanesQuery},
    {face_names(Sweep::Posteriors, Face::Windows), 511, 8, true, false, false, kOverLanes, kOverLanesQuery},
    {{"alignment_posteriors_lattice", "alignment_posteriors_lattice", "posterior_lattice"}, 4095, 16, true, true, false, kOverStrip, kOverStrip},
    {{"alignment_posteriors_repeats", "alignment_posteriors_repeats", "posterior_repeats"}, 511, 8, true, true, true, kOverLanes, kOverLanesQuery},
    {{"alignment_posteriors_song", "alignment_posteriors_song", "posterior_song"}, 4095, 16, true, true, true, kOverStrip, kOverStrip}};

int query_workspace(EntryId id, int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    const Entry &e = kEntries[id];
    LA_CHECK_ARG(bytes && batch >= 0 && max_frames > 0 && max_labels > 0, "%s_workspace_bytes: bad arguments", e.names.query);
    PostPlan pl;
    if (!plan_posterior(batch, max_frames, max_labels, e.label_limit, &pl, e.repeats)) {
        la::set_error(e.over_query, e.names.query, max_labels);
        return LA_EUNSUPPORTED;
    }
    *bytes = pl.ws_bytes();
    return LA_OK;
}

// the six la_alignment_posteriors* entry points: p holds the caller's arguments, null / zero standing in for what the entry does not
// have (Windows: skip_from may be null, skip_stride stays the row pitch of span_skip_prob); the workspace fields are set here.  The
// RepParams part is read for kRepeats and kSong only
int run_posteriors(EntryId id, RepParams p, int32_t batch, void *workspace, size_t workspace_bytes, hipStream_t stream) {
    const Entry &e = kEntries[id];
    const char *who = e.names.entry;
    if (batch == 0) return LA_OK;
    Face face = id >= kLattice ? Face::Plain : (Face)id;
    if (id >= kLattice) {
        LA_CHECK_ARG((p.win_lo == nullptr) == (p.win_hi == nullptr), "%s: win_lo and win_hi go together (both null: no windows)", who);
        face = p.win_lo ? Face::Windows : p.skip_from ? Face::Spans : Face::Plain;
    }
    LA_CHECK_ARG(p.inputs_present(face) && p.onset && p.offset, "%s: null input pointer", who);
    LA_CHECK_ARG(p.occupancy && p.onset_prob && p.offset_prob && p.log_z && p.status && (!e.span_outputs || (p.present_prob && p.span_skip_prob)),
                 "%s: null output pointer", who);
    LA_CHECK_ARG(p.sizes_ok(batch), "%s: bad sizes", who);
    LA_CHECK_ARG(p.window >= 0, "%s: negative boundary_window", who);
    // (la_alignment_posteriors has no penalty: 0.  The lattice entry checks the one it was given whatever the face)
    LA_CHECK_ARG(p.penalty >= 0.0, "%s: skip_penalty must be >= 0 (and not NaN)", who);
    if (e.repeats) {
        LA_CHECK_ARG(p.repeat_count, "%s: null output pointer", who);
        LA_CHECK_ARG(p.repeat_penalty >= 0.0, "%s: repeat_penalty must be >= 0 (and not NaN)", who);
        LA_CHECK_ARG(!p.path_prob || p.path, "%s: path_prob needs the path it is asked about", who);
    }
    PostPlan pl;
    const bool planned = plan_posterior(batch, p.max_frames, p.max_labels, e.label_limit, &pl, e.repeats);
    if (planned || !e.limit_first) {
        LA_CHECK_ARG(p.strides_ok(face, p.out_stride, true) && (!e.span_outputs || p.skip_stride >= p.max_labels + 1),
                     "%s: strides smaller than max_labels", who);
        LA_CHECK_ARG(!p.gamma || (p.gamma_rs >= 2 * (int64_t)p.max_labels + 1 && (batch == 1 || p.gamma_bs >= (int64_t)p.max_frames * p.gamma_rs)),
                     "%s: gamma strides smaller than [max_frames][2 max_labels + 1]", who);
        if (e.repeats) {
            LA_CHECK_ARG(!p.repeat_from || p.repeat_stride >= p.max_labels, "%s: repeat_stride smaller than max_labels", who);
            LA_CHECK_ARG(!(p.path || p.path_prob) || p.path_stride >= p.max_frames, "%s: path_stride smaller than max_frames", who);
        }
    }
    if (!planned) {
        la::set_error(e.over_entry, who, p.max_labels);
        return LA_EUNSUPPORTED;
    }
    const size_t need = pl.ws_bytes();
    LA_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
    LA_CHECK_ARG((uintptr_t)workspace % e.ws_align == 0, "%s: workspace must be %zu-byte aligned", who, e.ws_align);
    unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
    p.alpha_ws = reinterpret_cast<double *>(ws);
    if (pl.R) {
        p.acc_ws = reinterpret_cast<double *>(ws + pl.alpha_bytes);
        p.csr_ws = reinterpret_cast<int32_t *>(ws + pl.alpha_bytes + pl.acc_bytes);
    }
    if (e.repeats) return launch_repeats(pl.R ? e.names.timer : kEntries[kRepeats].names.timer, p, pl, batch, stream);
    const char *timer = pl.R ? e.names.timer : kEntries[(int)face].names.timer;
    int st = LA_EUNSUPPORTED;
    switch (face) {
        case Face::Plain: st = launch_face<false, false>(timer, p, pl, batch, stream); break;
        case Face::Spans: st = launch_face<true, false>(timer, p, pl, batch, stream); break;
        case Face::Windows: st = launch_face<true, true>(timer, p, pl, batch, stream); break;
    }
    if (st == LA_OK && e.span_outputs && face == Face::Plain && !pl.R) {
        hipLaunchKernelGGL(no_span_outputs_kernel, dim3(batch), dim3(256), 0, stream, p.status, p.n_labels, p.max_labels, p.present_prob,
                           p.out_stride, p.span_skip_prob, p.skip_stride);
        LA_LAUNCH_CHECK();
    }
    return st;
}

int run_posteriors(EntryId id, const PostParams &pp, int32_t batch, void *workspace, size_t workspace_bytes, hipStream_t stream) {
    RepParams p{};
    static_cast<PostParams &>(p) = pp;
    return run_posteriors(id, p, batch, workspace, workspace_bytes, stream);
}

// the caller's arguments of an entry point by name; null / zero stands in for what the entry does not have
PostParams shared_params(const float *em, int64_t em_batch_stride, int64_t em_row_stride, const int32_t *labels, int32_t labels_stride,
                         const int32_t *n_labels, const int32_t *n_frames, int32_t max_frames, int32_t max_labels, const int32_t *onset,
                         const int32_t *offset, int32_t out_stride, int32_t boundary_window, const int32_t *skip_from, int32_t skip_stride,
                         double skip_penalty, const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride, float *occupancy,
                         float *onset_prob, float *offset_prob, float *present_prob, float *span_skip_prob, double *log_z, int32_t *status,
                         float *gamma_out, int64_t gamma_batch_stride, int64_t gamma_row_stride) {
    PostParams p{};
    p.set_inputs(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels);
    p.set_spans(skip_from, skip_stride, skip_penalty);
    p.set_windows(win_lo, win_hi, win_stride);
    p.onset = onset, p.offset = offset, p.out_stride = out_stride, p.window = boundary_window;
    p.occupancy = occupancy, p.onset_prob = onset_prob, p.offset_prob = offset_prob;
    p.present_prob = present_prob, p.span_skip_prob = span_skip_prob;
    p.log_z = log_z, p.status = status;
    p.gamma = gamma_out, p.gamma_bs = gamma_batch_stride, p.gamma_rs = gamma_row_stride;
    return p;
}

}  // namespace

extern "C" int la_alignment_posteriors_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    return query_workspace(kPlain, batch, max_frames, max_labels, bytes);
}

extern "C" int la_alignment_posteriors_spans_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    return query_workspace(kSpans, batch, max_frames, max_labels, bytes);
}

extern "C" int la_alignment_posteriors_windows_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    return query_workspace(kWindows, batch, max_frames, max_labels, bytes);
}

extern "C" int la_alignment_posteriors_lattice_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    return query_workspace(kLattice, batch, max_frames, max_labels, bytes);
}

extern "C" int la_alignment_posteriors_repeats_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    return query_workspace(kRepeats, batch, max_frames, max_labels, bytes);
}

extern "C" int la_alignment_posteriors_song_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    return query_workspace(kSong, batch, max_frames, max_labels, bytes);
}

namespace {
// la_alignment_posteriors_repeats and la_alignment_posteriors_song: one argument list, two label limits
int run_repeat_entry(EntryId id, const float *em, int64_t em_batch_stride, int64_t em_row_stride, const int32_t *labels, int32_t labels_stride,
                     const int32_t *n_labels, const int32_t *n_frames, int32_t batch, int32_t max_frames, int32_t max_labels,
                     const int32_t *onset, const int32_t *offset, int32_t out_stride, int32_t boundary_window, const int32_t *skip_from,
                     int32_t skip_stride, double skip_penalty, const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride,
                     const int32_t *repeat_from, int32_t repeat_stride, double repeat_penalty, const int32_t *path, int32_t path_stride,
                     float *occupancy, float *onset_prob, float *offset_prob, float *visits, float *span_skip_prob, float *repeat_count,
                     float *path_prob, double *log_z, int32_t *status, float *gamma_out, int64_t gamma_batch_stride, int64_t gamma_row_stride,
                     void *workspace, size_t workspace_bytes, void *stream_) {
    RepParams p{};
    static_cast<PostParams &>(p) =
        shared_params(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels, onset, offset,
                      out_stride, boundary_window, skip_from, skip_stride, skip_penalty, win_lo, win_hi, win_stride, occupancy, onset_prob,
                      offset_prob, visits, span_skip_prob, log_z, status, gamma_out, gamma_batch_stride, gamma_row_stride);
    p.repeat_from = repeat_from, p.repeat_stride = repeat_stride, p.repeat_penalty = repeat_penalty;
    p.path = path, p.path_stride = path_stride, p.repeat_count = repeat_count, p.path_prob = path_prob;
    return run_posteriors(id, p, batch, workspace, workspace_bytes, (hipStream_t)stream_);
}
}  // namespace

extern "C" int la_alignment_posteriors_song(const float *em, int64_t em_batch_stride, int64_t em_row_stride, const int32_t *labels,
                                            int32_t labels_stride, const int32_t *n_labels, const int32_t *n_frames, int32_t batch,
                                            int32_t max_frames, int32_t max_labels, const int32_t *onset, const int32_t *offset,
                                            int32_t out_stride, int32_t boundary_window, const int32_t *skip_from, int32_t skip_stride,
                                            double skip_penalty, const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride,
                                            const int32_t *repeat_from, int32_t repeat_stride, double repeat_penalty,
                                            const int32_t *path, int32_t path_stride, float *occupancy, float *onset_prob,
                                            float *offset_prob, float *visits, float *span_skip_prob, float *repeat_count,
                                            float *path_prob, double *log_z, int32_t *status, float *gamma_out,
                                            int64_t gamma_batch_stride, int64_t gamma_row_stride, void *workspace,
                                            size_t workspace_bytes, void *stream_) {
    return run_repeat_entry(kSong, em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, batch, max_frames,
                            max_labels, onset, offset, out_stride, boundary_window, skip_from, skip_stride, skip_penalty, win_lo, win_hi,
                            win_stride, repeat_from, repeat_stride, repeat_penalty, path, path_stride, occupancy, onset_prob, offset_prob,
                            visits, span_skip_prob, repeat_count, path_prob, log_z, status, gamma_out, gamma_batch_stride, gamma_row_stride,
                            workspace, workspace_bytes, stream_);
}

extern "C" int la_alignment_posteriors_repeats(const float *em, int64_t em_batch_stride, int64_t em_row_stride, const int32_t *labels,
                                               int32_t labels_stride, const int32_t *n_labels, const int32_t *n_frames, int32_t batch,
                                               int32_t max_frames, int32_t max_labels, const int32_t *onset, const int32_t *offset,
                                               int32_t out_stride, int32_t boundary_window, const int32_t *skip_from, int32_t skip_stride,
                                               double skip_penalty, const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride,
                                               const int32_t *repeat_from, int32_t repeat_stride, double repeat_penalty,
                                               const int32_t *path, int32_t path_stride, float *occupancy, float *onset_prob,
                                               float *offset_prob, float *visits, float *span_skip_prob, float *repeat_count,
                                               float *path_prob, double *log_z, int32_t *status, float *gamma_out,
                                               int64_t gamma_batch_stride, int64_t gamma_row_stride, void *workspace,
                                               size_t workspace_bytes, void *stream_) {
    return run_repeat_entry(kRepeats, em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, batch, max_frames,
                            max_labels, onset, offset, out_stride, boundary_window, skip_from, skip_stride, skip_penalty, win_lo, win_hi,
                            win_stride, repeat_from, repeat_stride, repeat_penalty, path, path_stride, occupancy, onset_prob, offset_prob,
                            visits, span_skip_prob, repeat_count, path_prob, log_z, status, gamma_out, gamma_batch_stride, gamma_row_stride,
                            workspace, workspace_bytes, stream_);
}

extern "C" int la_alignment_posteriors(const float *em, int64_t em_batch_stride, int64_t em_row_stride, const int32_t *labels,
                                       int32_t labels_stride, const int32_t *n_labels, const int32_t *n_frames, int32_t batch,
                                       int32_t max_frames, int32_t max_labels, const int32_t *onset, const int32_t *offset,
                                       int32_t out_stride, int32_t boundary_window, float *occupancy, float *onset_prob,
                                       float *offset_prob, double *log_z, int32_t *status, float *gamma_out,
                                       int64_t gamma_batch_stride, int64_t gamma_row_stride, void *workspace,
                                       size_t workspace_bytes, void *stream_) {
    return run_posteriors(kPlain,
                          shared_params(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels,
                                        onset, offset, out_stride, boundary_window, nullptr, 0, 0.0, nullptr, nullptr, 0, occupancy, onset_prob,
                                        offset_prob, nullptr, nullptr, log_z, status, gamma_out, gamma_batch_stride, gamma_row_stride),
                          batch, workspace, workspace_bytes, (hipStream_t)stream_);
}

extern "C" int la_alignment_posteriors_spans(const float *em, int64_t em_batch_stride, int64_t em_row_stride, const int32_t *labels,
                                             int32_t labels_stride, const int32_t *n_labels, const int32_t *n_frames, int32_t batch,
                                             int32_t max_frames, int32_t max_labels, const int32_t *onset, const int32_t *offset,
                                             int32_t out_stride, int32_t boundary_window, const int32_t *skip_from, int32_t skip_stride,
                                             double skip_penalty, float *occupancy, float *onset_prob, float *offset_prob,
                                             float *present_prob, float *span_skip_prob, double *log_z, int32_t *status, float *gamma_out,
                                             int64_t gamma_batch_stride, int64_t gamma_row_stride, void *workspace,
                                             size_t workspace_bytes, void *stream_) {
    return run_posteriors(kSpans,
                          shared_params(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels,
                                        onset, offset, out_stride, boundary_window, skip_from, skip_stride, skip_penalty, nullptr, nullptr, 0,
                                        occupancy, onset_prob, offset_prob, present_prob, span_skip_prob, log_z, status, gamma_out,
                                        gamma_batch_stride, gamma_row_stride),
                          batch, workspace, workspace_bytes, (hipStream_t)stream_);
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
    return run_posteriors(kWindows,
                          shared_params(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels,
                                        onset, offset, out_stride, boundary_window, skip_from, skip_stride, skip_penalty, win_lo, win_hi,
                                        win_stride, occupancy, onset_prob, offset_prob, present_prob, span_skip_prob, log_z, status, gamma_out,
                                        gamma_batch_stride, gamma_row_stride),
                          batch, workspace, workspace_bytes, (hipStream_t)stream_);
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
    return run_posteriors(kLattice,
                          shared_params(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels,
                                        onset, offset, out_stride, boundary_window, skip_from, skip_stride, skip_penalty, win_lo, win_hi,
                                        win_stride, occupancy, onset_prob, offset_prob, present_prob, span_skip_prob, log_z, status, gamma_out,
                                        gamma_batch_stride, gamma_row_stride),
                          batch, workspace, workspace_bytes, (hipStream_t)stream_);
}
