// la_viterbi.hip -- batched forced-alignment DP for gfx950, on the reference's lattice and on the lattice with OPTIONAL label spans.
//
// Replaces utils/alignment.py:73-119 (run_viterbi_core) and :141-185 (init,
// termination, backtrace, first/last frame per label) of the reference.
//
// Mapping to the hardware (DESIGN.md "Viterbi"): the recurrence reads only row
// j-1, so one workgroup sweeps one utterance row by row with one lane per
// lattice state k (S = 2L+1 states).  For S <= 64 (every Opencpop utterance and
// the 30 s benchmark clips) that is ONE wave64 and the k-1 / k-2 neighbours come
// from DPP wave shifts, no LDS and no barrier in the loop.  Larger lattices
// (long-form songs) use up to 16 waves and a double-buffered f64 row in LDS with
// one barrier per frame.  Scores are float64, comparisons are in the reference's
// order; backpointers are the offsets {0,1,2} packed as two 64-bit ballot masks
// per wave per frame and kept in LDS when they fit (T * 16 B per wave), otherwise
// in the caller's workspace.  The kernel is latency-bound (T dependent steps),
// not bandwidth-bound: emissions are prefetched PF frames ahead into registers.
//
// Optional spans (the SPANS instantiations, la_viterbi_spans_batch; no counterpart in the reference, whose lattice makes every
// label occupy at least one frame).  States: 0 = leading silence, 2n+1 = label n, 2n+2 = the silence after it.  skip_from[n] = a
// with 0 <= a < n declares labels a .. n-1 optional: the two states at position n (2n, and 2n+1 when n < L) get two more
// predecessors, J = 2a (the silence before the span) and J-1 = 2a-1 (the label before it; a >= 1, and for the odd target
// only when labels[n] != labels[a-1] -- the equal-neighbour rule).  Both are charged `penalty` and must beat the existing
// rule's winner strictly, J before J-1.  Float64 adds / subtracts in that order: results are reproducible to the bit.
// The single-wave form fetches the jump sources with ds_bpermute of p0 and of the already-shifted p1 (lane J of p1 holds
// dp[J-1]); the multi-wave forms read dp[J] / dp[J-1] from the LDS row they exchange anyway.  "This clip has a span" is a
// workgroup-uniform test taken ONCE, outside the frame loop: a span-free clip runs the loop of the plain DP, without any of the
// jump code.  Backpointers are then five outcomes {stay, advance, skip, jump from J, jump from J-1}: three ballot masks per wave
// per frame (T * 24 B per wave; the third is written and read only where spans exist), and J(s) stays in an LDS int array for
// the backtrace thread.
//
// Frame windows (the WIN instantiations, la_viterbi_windows_batch): state s may hold the path at frame t only if lo[s] <= t < hi[s];
// a cell outside its window is -inf.  Each lane keeps its state's lo / hi in two registers.  The test depends on the frame index
// alone, so it is applied to the EMISSION as it leaves the prefetch registers (e = inside ? e : -inf, and likewise to row 0):
// best + (double)e is then -inf without an instruction on the loop-carried chain (best is never +inf or NaN).  WIN exists only
// together with SPANS (a null skip_from = no span anywhere; the once-per-clip has_span test still sends a span-free clip through the
// plain loop).  A winning final score of -inf is LA_EINFEASIBLE with every onset / offset -1; otherwise backtrace and status are
// unchanged.
//
// More than 511 labels (la_viterbi_lattice_batch): the span and window faces of viterbi_strip_kernel, described there.
//
// Repeatable spans (the REP instantiations, la_viterbi_repeats_batch): a line sung more often than printed.  repeat_from[a] = e with
// a < e <= L lets the path return to label a after label e-1: the odd state 2a+1 gets two more predecessors from the previous frame,
// K = 2e (the silence after the span, always) and K-1 = 2e-1 (label e-1, only when labels[a] != labels[e-1]).  The DP is
// frame-synchronous, so an arc to the left makes no cycle; it is the skip arcs' fetch with a source to the right of the target
// (ds_bpermute in the one-wave form, the LDS row elsewhere; repeat_source in la_lattice.h is the rule, beside span_source).  Order per
// cell: the existing rule, J, J-1, then K and K-1 (each charged repeat_penalty, each only if strictly greater), the emission last.
// Backpointer codes 5 and 6 fit the three ballot words of the span faces.  REP exists only on top of SPANS + WIN with null pointers
// meaning "absent"; the once-per-clip test reads "a span or a repeat arc", so a clip with neither runs the plain loop.  The path is no
// longer monotone: the backtrace writes the state of every frame to `path`, onset / offset are those of a label's FIRST visit in time,
// and a label inside a taken skip jump on one pass and visited on another keeps its visit (the kSkipped mark goes to on_s, only where
// there is no visit yet, and a visit overwrites it); the backtrace thread recomputes K(kk) from repeat_from.
#include <type_traits>

#include "la_lattice_tile.h"

namespace {

using namespace la::lattice;

constexpr int PF = 8;                 // emission prefetch depth (frames)
constexpr int kSkipped = -2;          // off_s marker of a label inside a taken jump (written out as -1); the repeat face marks on_s / onset

struct VitParams : LatticeIn {
    int32_t *onset, *offset;
    int32_t out_stride;
    double *final_score;
    int32_t *status;
    unsigned long long *bt_global;  // [batch][max_frames][NW][2, with spans 3] when !bt_in_lds
    int32_t bt_in_lds;
    // run_viterbi_core face (DUMP instantiation only, batch 1): row 0 of dp is READ, rows >= 1 of dp / bt are written
    double *dp_dump;    // [T][S]
    long long *bt_dump; // [T][S]
    // repeatable spans (REP instantiations only): repeat_from [batch][repeat_stride], entries 0 .. L_b - 1 of row b are read; null = none
    const int32_t *repeat_from;
    int32_t repeat_stride;
    double repeat_penalty;
    int32_t *path;      // [batch][path_stride]: the state at every frame (REP instantiations only); null = not wanted
    int32_t path_stride;

    void set_outputs(int32_t *onset_, int32_t *offset_, int32_t out_stride_, double *final_score_, int32_t *status_) {
        onset = onset_, offset = offset_, out_stride = out_stride_, final_score = final_score_, status = status_;
    }
};

// The recurrence cell of both kernels is la_lattice_tile.h's Cell / choose_neighbour; their jumps add the codes 3 jump from J, 4 jump from
// J-1; 5 repeat from K, 6 from K-1.
// The two arcs of the span that ends at this state (J >= 0): each is charged pen and must beat the winner so far STRICTLY, J before J-1.
// dp_jm1 is dereferenced only where that arc exists.  C0 = 5: the same rule for the two arcs of the repeat span that starts at this
// state (sources K, K-1, codes 5 and 6), applied after the skip span's.
template <int C0 = 3>
__device__ __forceinline__ Cell jump_step(Cell c, const double *dp_j, const double *dp_jm1, bool jm1_ok, double pen) {
    const double vj = *dp_j - pen;
    if (vj > c.best) c = {C0, vj};
    if (jm1_ok) {
        const double vm = *dp_jm1 - pen;
        if (vm > c.best) c = {C0 + 1, vm};
    }
    return c;
}

template <int NW, bool DPP, bool SPANS, bool DUMP = false, bool WIN = false, bool REP = false>
__global__ __launch_bounds__(NW * 64) void viterbi_kernel(VitParams p) {
    static_assert(!REP || WIN, "repeatable spans are a face of the span + window forms (null pointers: absent)");
    static_assert(!DPP || NW == 1, "DPP neighbour exchange is single-wave only");
    static_assert(!DUMP || (!DPP && !SPANS), "the dp / bt dump is a face of the plain LDS-exchange form");
    static_assert(!WIN || (SPANS && !DUMP), "frame windows are a face of the optional-span forms");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NT = NW * 64;
    constexpr int MW = SPANS ? 3 : 2;  // backpointer mask words per wave per frame
    // carve: row exchange [2][NT+2] f64 | on/off [2][max_labels] i32 | with spans: J [NT] i32 | bt masks
    double *rowbuf = reinterpret_cast<double *>(smem);
    int32_t *on_s = reinterpret_cast<int32_t *>(smem + 2 * (NT + 2) * sizeof(double));
    const int Lpad = (p.max_labels + 3) & ~3;
    int32_t *off_s = on_s + Lpad;
    int32_t *j_s = off_s + Lpad;
    unsigned long long *bt_lds = reinterpret_cast<unsigned long long *>(j_s + (SPANS ? NT : 0));

    const int b = blockIdx.x;
    const int k = threadIdx.x;
    const int wave = k >> 6;
    const int lane = k & 63;
    const int L = p.n_labels[b];
    const int T = p.n_frames[b];
    const int S = 2 * L + 1;

    for (int n = k; n < p.max_labels; n += NT) {
        p.onset[(int64_t)b * p.out_stride + n] = -1;
        p.offset[(int64_t)b * p.out_stride + n] = -1;
        on_s[n] = -1;
        off_s[n] = -1;
    }
    [[maybe_unused]] int32_t *path_b = nullptr;   // every frame -1 until the backtrace has been there
    if constexpr (REP) {
        if (p.path) {
            path_b = p.path + (int64_t)b * p.path_stride;
            for (int t = k; t < p.max_frames; t += NT) path_b[t] = -1;
        }
    }
    if (L <= 0) {  // reference: IndexError at cur_label[0] (:152)
        if (k == 0) { p.status[b] = LA_EEMPTY; p.final_score[b] = 0.0; }
        return;
    }
    if (T <= 0 || T > p.max_frames || L > p.max_labels || S > NT) {
        if (k == 0) { p.status[b] = LA_EINVAL; p.final_score[b] = 0.0; }
        return;
    }

    unsigned long long *bt = p.bt_in_lds ? bt_lds : p.bt_global + (int64_t)b * p.max_frames * NW * MW;

    const bool valid = k < S;
    const bool odd = (k & 1) != 0;
    const int n = k >> 1;
    const int col = (odd && valid) ? 1 + n : 0;
    const int32_t *lab = p.labels + (int64_t)b * p.labels_stride;
    bool can_skip = false;  // label[k//2] != label[k//2-1], odd k >= 3 (:104)
    if (odd && valid && k >= 3) can_skip = lab[n] != lab[n - 1];
    // the span that ends at this state's position n (n <= L for every valid state); anything outside 0 <= a < n is "none"
    int J = -1;
    bool jm1_ok = false;
    if constexpr (SPANS) {
        // (windows: a null skip_from = no span anywhere)
        const SpanSource src = span_source(!WIN || p.skip_from ? p.skip_from + (int64_t)b * p.skip_stride : nullptr, lab, k, valid);
        J = src.J;
        jm1_ok = src.jm1_ok;
        j_s[k] = J;
    }
    // the repeat span that starts at this state's label (odd states only)
    [[maybe_unused]] int K = -1;
    [[maybe_unused]] bool km1_ok = false;
    [[maybe_unused]] const int32_t *rep_b = nullptr;
    if constexpr (REP) {
        if (p.repeat_from) rep_b = p.repeat_from + (int64_t)b * p.repeat_stride;
        const RepeatSource src = repeat_source(rep_b, lab, k, valid, L);
        K = src.K;
        km1_ok = src.km1_ok;
    }
    [[maybe_unused]] const double rpen = p.repeat_penalty;
    const double pen = p.penalty;
    const float *emb = p.em + (int64_t)b * p.em_bs + col;
    // this state's frame window; lanes without a state keep the open one (nothing is read past 2 L_b <= win_stride - 1)
    int wlo = 0, whi = 0x7fffffff;
    if constexpr (WIN) {
        if (valid && (!REP || p.win_lo)) {   // (repeats: a null window pair = every window open)
            wlo = p.win_lo[(int64_t)b * p.win_stride + k];
            whi = p.win_hi[(int64_t)b * p.win_stride + k];
        }
    }
    auto gated = [&](float e, int j) { return (j >= wlo && j < whi) ? e : -INFINITY; };

    // row 0 (:144-152); the run_viterbi_core face takes row 0 from the caller like the reference does (:73-76)
    double cur = (k <= 1) ? (double)emb[0] : kNeg;
    if (DUMP) cur = valid ? p.dp_dump[k] : kNeg;
    if constexpr (WIN) {
        if (!(0 >= wlo && 0 < whi)) cur = -INFINITY;
    }

    if (!DPP) {
        if (k < 2) { rowbuf[k] = kNeg; rowbuf[NT + 2 + k] = kNeg; }  // slots for k-1, k-2 of states 0,1
    }
    // workgroup-uniform (one wave: a ballot): a clip without a span runs a frame loop without any of the jump code
    // (repeats: neither a span nor a repeat arc; has_span then reads "has a jump of either kind")
    const bool has_span = SPANS && (NW == 1 ? __ballot(J >= 0 || K >= 0) != 0ull : __syncthreads_or(J >= 0 || K >= 0) != 0);
    const int gather_addr = (J >= 0 ? J : lane) << 2;   // (single wave: J < S <= 64)
    [[maybe_unused]] const int gather_addr_k = (K >= 0 ? K : lane) << 2;   // (K <= 2 L < S)

    float e_buf[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        const int jj = 1 + i;
        e_buf[i] = jj < T ? emb[(int64_t)jj * p.em_rs] : 0.0f;
    }
    int parity = 0;
    auto sweep = [&](auto has_c) {
        constexpr bool HAS = decltype(has_c)::value;  // this clip has a span
        for (int j0 = 1; j0 < T; j0 += PF) {
            float e_cur[PF];
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                if constexpr (WIN) e_cur[i] = gated(e_buf[i], j0 + i);   // the window's gate: off the dependent chain
                else e_cur[i] = e_buf[i];
            }
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const int jj = j0 + PF + i;
                e_buf[i] = jj < T ? emb[(int64_t)jj * p.em_rs] : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const int j = j0 + i;
                if (j >= T) break;
                double p0 = cur, p1, p2, pj = kNeg, pjm1 = kNeg;
                [[maybe_unused]] double pk = kNeg, pkm1 = kNeg;
                if (DPP) {
                    p1 = wave_shr1(p0, 0.0);
                    p2 = wave_shr1(p1, 0.0);
                    if (HAS) {
                        pj = wave_gather(p0, gather_addr);
                        pjm1 = wave_gather(p1, gather_addr);   // lane J of the shifted row holds dp[J-1]
                        if constexpr (REP) {                   // a source to the right of the target: the same fetch
                            pk = wave_gather(p0, gather_addr_k);
                            pkm1 = wave_gather(p1, gather_addr_k);
                        }
                    }
                } else {
                    double *rb = rowbuf + parity * (NT + 2);
                    rb[k + 2] = p0;
                    __syncthreads();
                    p1 = rb[k + 1];
                    p2 = rb[k];
                    if (HAS && J >= 0) {
                        pj = rb[J + 2];
                        pjm1 = rb[J + 1];
                    }
                    if constexpr (REP) {
                        if (HAS && K >= 0) {
                            pk = rb[K + 2];
                            pkm1 = rb[K + 1];
                        }
                    }
                    parity ^= 1;
                }
                Cell c = choose_neighbour(p0, p1, p2, can_skip, k == 0);
                if (HAS && J >= 0) c = jump_step(c, &pj, &pjm1, jm1_ok, pen);
                if constexpr (REP) {
                    if (HAS && K >= 0) c = jump_step<5>(c, &pk, &pkm1, km1_ok, rpen);
                }
                const int code = c.code;
                cur = c.best + (double)e_cur[i];
                if (DUMP && valid) {
                    p.dp_dump[(int64_t)j * S + k] = cur;
                    p.bt_dump[(int64_t)j * S + k] = k - code;
                }
                const unsigned long long m0 = __ballot(code & 1);
                const unsigned long long m1 = __ballot((code >> 1) & 1);
                unsigned long long m2 = 0ull;
                if (HAS) m2 = __ballot(code >> 2);
                if (lane == 0) {
                    unsigned long long *row = bt + ((int64_t)j * NW + wave) * MW;
                    row[0] = m0;
                    row[1] = m1;
                    if (HAS) row[2] = m2;                                    // (read back only for states with a span)
                }
            }
        }
    };
    if (has_span) sweep(std::bool_constant<SPANS>{});
    else sweep(std::false_type{});

    // termination + backtrace (:157-185) by one thread
    __syncthreads();
    double *fin = rowbuf;
    fin[k] = cur;
    __threadfence_block();
    __syncthreads();
    if (k == 0) {
        int kk = (fin[S - 1] > fin[S - 2]) ? (S - 1) : (S - 2);  // strict '>' (:157)
        p.final_score[b] = fin[kk];
        int knext = -1;
        const bool no_path = WIN && fin[kk] == -INFINITY;   // no path inside the windows: on_s / off_s stay -1, no backtrace
        for (int j = no_path ? -1 : T - 1; j >= 0; --j) {
            if (kk & 1) {
                const int nn = kk >> 1;
                if (kk != knext) off_s[nn] = j + 1;  // last frame in this state + 1
                on_s[nn] = j;                        // keeps decreasing to the first frame
            }
            if constexpr (REP) {
                if (path_b) path_b[j] = kk;
            }
            knext = kk;
            if (j > 0) {
                const unsigned long long *row = bt + ((int64_t)j * NW + (kk >> 6)) * MW;
                const int sh = kk & 63;
                int code = (int)((row[0] >> sh) & 1ull) | ((int)((row[1] >> sh) & 1ull) << 1);
                if constexpr (REP) {
                    // The path is no longer monotone: a label inside a taken skip jump on one pass may be visited on another, and then the
                    // visit wins.  A taken jump marks on_s = kSkipped only where the label has no visit so far, and a visit (above, at an
                    // earlier frame) overwrites the mark; the onset / offset left at the end are those of the FIRST visit in time.
                    if (has_span) {                      // (uniform; with a jump of either kind the third mask covers every state)
                        code |= (int)((row[2] >> sh) & 1ull) << 2;
                        if (code >= 5) {
                            const int Kk = repeat_source(rep_b, lab, kk, true, L).K;   // recomputed, as the strip kernel recomputes J
                            code = kk - (Kk - (code - 5));                            // (negative: the predecessor lies to the right)
                        } else if (code >= 3) {
                            const int Jk = j_s[kk];
                            for (int m = Jk >> 1; m < (kk >> 1); ++m)
                                if (on_s[m] == -1) on_s[m] = kSkipped;
                            code = kk - (Jk - (code - 3));
                        }
                    }
                } else if constexpr (SPANS) {
                    if (has_span) {                      // (uniform: a span-free clip's backtrace is the plain DP's)
                        const int Jk = j_s[kk];          // the third mask exists only where spans do
                        if (Jk >= 0) code |= (int)((row[2] >> sh) & 1ull) << 2;
                        if (code >= 3) {
                            for (int m = Jk >> 1; m < (kk >> 1); ++m) off_s[m] = kSkipped;
                            code = kk - (Jk - (code - 3));
                        }
                    }
                }
                kk -= code;
            }
        }
        int st = LA_OK;
        for (int nn = 0; nn < L; ++nn) {
            if (REP && on_s[nn] == kSkipped) on_s[nn] = -1;    // (never visited: off_s is still -1)
            else if (!REP && SPANS && off_s[nn] == kSkipped) off_s[nn] = -1;
            else if (on_s[nn] < 0) st = LA_EINFEASIBLE;  // reference: ValueError from list.index (:183)
        }
        p.status[b] = st;   // (no path inside the windows: every on_s is -1, so LA_EINFEASIBLE)
    }
    __syncthreads();
    for (int nn = k; nn < L; nn += NT) {
        p.onset[(int64_t)b * p.out_stride + nn] = on_s[nn];
        p.offset[(int64_t)b * p.out_stride + nn] = off_s[nn];
    }
}

// Lattices beyond 1024 states (whole songs with more than 511 characters; the reference's run_viterbi_core has no limit):
// 1024 threads, each owning R CONSECUTIVE states k = tid*R + r, so 1024*R states per workgroup (R = 2, 4, 8 -> up to 4095
// labels).  Same recurrence, same comparison order, float64; the previous row goes through a double-buffered f64 row in
// LDS (one barrier per frame).  Backpointer masks: [frame][r][wave][2] 64-bit ballots in the caller's workspace.
// Onset / offset go straight to the outputs (no LDS copies: the row buffers take the LDS at R = 8).
// The SPANS and SPANS + WIN faces (la_viterbi_lattice_batch beyond 511 labels) are viterbi_kernel's on this form.  A jump source J
// or J-1 can be any state of any thread, one of the reading thread's own included, so where the clip has a span (workgroup-uniform,
// tested once outside the frame loop) every thread writes ALL R of its states into the row of the current parity and reads dp[J] /
// dp[J-1] from that row after the barrier -- never from cur[], which the same r loop is overwriting.  A span-free clip runs the
// plain loop: two row states, two mask words, no jump code.  J, jm1_ok and the window pair of each owned state stay in registers
// (the two rows take 131,104 B of LDS at R = 8: no room for a J array); the backtrace thread recomputes J(kk) from skip_from.
// Masks are then [frame][r][wave][3], the third word written and read only where the clip has a span.  The window's gate is applied
// to the emission as it leaves the prefetch registers, off the loop-carried chain, as in viterbi_kernel.
template <int R, bool SPANS = false, bool WIN = false, bool REP = false>
__global__ __launch_bounds__(1024) void viterbi_strip_kernel(VitParams p) {
    static_assert(!WIN || SPANS, "frame windows are a face of the optional-span forms");
    static_assert(!REP || WIN, "repeatable spans are a face of the span + window forms (null pointers: absent)");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // (R = 8 with spans: J, the window pairs and two generations of 4 x 8 prefetched emissions do not fit 128 VGPRs; the face waits on
    // the barrier, not on the loads, so its prefetch is two frames deep, and one frame deep with the 16 window registers)
    constexpr int NT = 1024, NS = NT * R, SPF = R < 8 || !SPANS ? 4 : WIN ? 1 : 2;
    constexpr int MW = SPANS ? 3 : 2;  // backpointer mask words per (frame, r, wave)
    double *rowbuf = reinterpret_cast<double *>(smem);      // [2][NS + 2]
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int L = p.n_labels[b];
    const int T = p.n_frames[b];
    const int S = 2 * L + 1;
    int32_t *on_g = p.onset + (int64_t)b * p.out_stride, *off_g = p.offset + (int64_t)b * p.out_stride;
    for (int n = tid; n < p.max_labels; n += NT) { on_g[n] = -1; off_g[n] = -1; }
    [[maybe_unused]] int32_t *path_b = nullptr;   // every frame -1 until the backtrace has been there
    if constexpr (REP) {
        if (p.path) {
            path_b = p.path + (int64_t)b * p.path_stride;
            for (int t = tid; t < p.max_frames; t += NT) path_b[t] = -1;
        }
    }
    if (L <= 0) {
        if (tid == 0) { p.status[b] = LA_EEMPTY; p.final_score[b] = 0.0; }
        return;
    }
    if (T <= 0 || T > p.max_frames || L > p.max_labels || S > NS) {
        if (tid == 0) { p.status[b] = LA_EINVAL; p.final_score[b] = 0.0; }
        return;
    }
    unsigned long long *bt = p.bt_global + (int64_t)b * p.max_frames * R * (16 * MW);
    const int32_t *lab = p.labels + (int64_t)b * p.labels_stride;
    const int k0 = tid * R;
    int col[R];
    bool can_skip[R], valid[R];
    double cur[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int k = k0 + r, n = k >> 1;
        valid[r] = k < S;
        const bool odd = (k & 1) != 0;
        col[r] = (odd && valid[r]) ? 1 + n : 0;
        can_skip[r] = odd && valid[r] && k >= 3 && lab[n] != lab[n - 1];
    }
    // the span that ends at each owned state's position, and each owned state's frame window (states >= S: none, the open window)
    [[maybe_unused]] const int32_t *skip_b = nullptr;
    [[maybe_unused]] int J[SPANS ? R : 1];
    [[maybe_unused]] bool jm1_ok[SPANS ? R : 1];
    [[maybe_unused]] int wlo[WIN ? R : 1], whi[WIN ? R : 1];
    [[maybe_unused]] bool has_span = false;
    // the repeat span that starts at each owned ODD state's label (k0 is even: the odd states are r = 2 h + 1)
    [[maybe_unused]] const int32_t *rep_b = nullptr;
    [[maybe_unused]] int K[REP ? R / 2 : 1];
    [[maybe_unused]] bool km1_ok[REP ? R / 2 : 1];
    if constexpr (SPANS) {
        if (!WIN || p.skip_from) skip_b = p.skip_from + (int64_t)b * p.skip_stride;   // (windows: a null skip_from = no span anywhere)
        bool any = false;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const SpanSource src = span_source(skip_b, lab, k0 + r, valid[r]);
            J[r] = src.J;
            jm1_ok[r] = src.jm1_ok;
            any |= src.J >= 0;
        }
        if constexpr (REP) {
            if (p.repeat_from) rep_b = p.repeat_from + (int64_t)b * p.repeat_stride;
#pragma unroll
            for (int h = 0; h < R / 2; ++h) {
                const RepeatSource src = repeat_source(rep_b, lab, k0 + 2 * h + 1, valid[2 * h + 1], L);
                K[h] = src.K;
                km1_ok[h] = src.km1_ok;
                any |= src.K >= 0;
            }
        }
        has_span = __syncthreads_or(any) != 0;   // workgroup-uniform: a clip without a span (repeats: without any jump) runs the plain loop
    }
    if constexpr (WIN) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            wlo[r] = 0, whi[r] = 0x7fffffff;
            if (valid[r] && (!REP || p.win_lo)) {   // (repeats: a null window pair = every window open)
                wlo[r] = p.win_lo[(int64_t)b * p.win_stride + k0 + r];
                whi[r] = p.win_hi[(int64_t)b * p.win_stride + k0 + r];
            }
        }
    }
    [[maybe_unused]] const double pen = p.penalty;
    [[maybe_unused]] const double rpen = p.repeat_penalty;
    const float *emb = p.em + (int64_t)b * p.em_bs;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        cur[r] = (k0 + r <= 1) ? (double)emb[col[r]] : kNeg;
        if constexpr (WIN) {
            if (!(0 >= wlo[r] && 0 < whi[r])) cur[r] = -INFINITY;
        }
    }
    if (tid == 0) { rowbuf[0] = kNeg; rowbuf[1] = kNeg; rowbuf[NS + 2] = kNeg; rowbuf[NS + 3] = kNeg; }

    float e_buf[SPF][R];
#pragma unroll
    for (int i = 0; i < SPF; ++i)
#pragma unroll
        for (int r = 0; r < R; ++r) e_buf[i][r] = (1 + i) < T ? emb[(int64_t)(1 + i) * p.em_rs + col[r]] : 0.0f;
    int parity = 0;
    auto sweep = [&](auto has_c) {
        constexpr bool HAS = decltype(has_c)::value;  // this clip has a span
        for (int j0 = 1; j0 < T; j0 += SPF) {
            float e_cur[SPF][R];
#pragma unroll
            for (int i = 0; i < SPF; ++i)
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if constexpr (WIN) e_cur[i][r] = (j0 + i >= wlo[r] && j0 + i < whi[r]) ? e_buf[i][r] : -INFINITY;   // the window's gate
                    else e_cur[i][r] = e_buf[i][r];
                }
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
                double *rb = rowbuf + parity * (NS + 2);
                if constexpr (HAS) {
                    // any state can be a jump source: the whole row goes through LDS
#pragma unroll
                    for (int r = 0; r < R; ++r) rb[k0 + 2 + r] = cur[r];
                } else {
                    // the two rightmost states of this thread are the k-1 / k-2 neighbours of the next thread's first states
                    rb[k0 + 2 + R - 1] = cur[R - 1];
                    rb[k0 + 2 + R - 2] = cur[R - 2];
                }
                __syncthreads();
                double prev[R + 2];
                prev[0] = rb[k0];
                prev[1] = rb[k0 + 1];
#pragma unroll
                for (int r = 0; r < R; ++r) prev[r + 2] = cur[r];
                parity ^= 1;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    Cell c = choose_neighbour(prev[r + 2], prev[r + 1], prev[r], can_skip[r], k0 + r == 0);
                    if constexpr (HAS) {
                        if (J[r] >= 0) c = jump_step(c, rb + J[r] + 2, rb + J[r] + 1, jm1_ok[r], pen);   // from the row, never from cur[]
                        if constexpr (REP) {
                            if ((r & 1) && K[r >> 1] >= 0) c = jump_step<5>(c, rb + K[r >> 1] + 2, rb + K[r >> 1] + 1, km1_ok[r >> 1], rpen);
                        }
                    }
                    const int code = c.code;
                    cur[r] = c.best + (double)e_cur[i][r];
                    const unsigned long long m0 = __ballot(code & 1);
                    const unsigned long long m1 = __ballot((code >> 1) & 1);
                    [[maybe_unused]] unsigned long long m2 = 0ull;
                    if constexpr (HAS) m2 = __ballot(code >> 2);
                    if (lane == 0) {
                        unsigned long long *row = bt + (((int64_t)j * R + r) * 16 + wave) * MW;
                        row[0] = m0;
                        row[1] = m1;
                        if constexpr (HAS) row[2] = m2;                                 // (read back only for states with a span)
                    }
                }
            }
        }
    };
    // (MW is this instantiation's: the plain kernels run sweep(false) at two mask words of pitch, a span-free clip of the span faces at three)
    if (has_span) sweep(std::bool_constant<SPANS>{});
    else sweep(std::false_type{});
    // termination + backtrace by one thread; the masks were written by other waves of this workgroup: drain + barrier first
    __syncthreads();
    double *fin = rowbuf;
#pragma unroll
    for (int r = 0; r < R; ++r) fin[k0 + r] = cur[r];
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        int kk = (fin[S - 1] > fin[S - 2]) ? (S - 1) : (S - 2);
        p.final_score[b] = fin[kk];
        int knext = -1, entered = 0, skipped = 0;
        const bool no_path = WIN && fin[kk] == -INFINITY;   // no path inside the windows: every onset / offset stays -1, no backtrace
        for (int j = no_path ? -1 : T - 1; j >= 0; --j) {
            if (kk & 1) {
                const int nn = kk >> 1;
                if (kk != knext) { off_g[nn] = j + 1; ++entered; }
                if (j == 0) on_g[nn] = 0;
            }
            if constexpr (REP) {
                if (path_b) path_b[j] = kk;
            }
            int knew = kk;
            if (j > 0) {
                const int t2 = kk / R, r = kk - t2 * R;
                const unsigned long long *row = bt + (((int64_t)j * R + r) * 16 + (t2 >> 6)) * MW;
                const int sh = t2 & 63;
                int code = (int)((row[0] >> sh) & 1ull) | ((int)((row[1] >> sh) & 1ull) << 1);
                if constexpr (REP) {
                    // No monotone path, so no entered + skipped count: a taken skip jump marks on_g = kSkipped only where the label has no
                    // visit so far, a visit at an earlier frame overwrites the mark (the visit wins), and the status is taken from on_g below.
                    if (has_span) {                          // (uniform; with a jump of either kind the third mask covers every state)
                        code |= (int)((row[2] >> sh) & 1ull) << 2;
                        if (code >= 5) {
                            const int Kk = repeat_source(rep_b, lab, kk, true, L).K;   // K(kk), as the sweep computed it
                            code = kk - (Kk - (code - 5));                            // (negative: the predecessor lies to the right)
                        } else if (code >= 3) {
                            const int ak = span_first(skip_b, kk >> 1);                // (code >= 3 only where the sweep saw a span: skip_b is not null)
                            for (int m = ak; m < (kk >> 1); ++m)
                                if (on_g[m] == -1) on_g[m] = kSkipped;
                            code = kk - (2 * ak - (code - 3));
                        }
                    }
                } else if constexpr (SPANS) {
                    if (has_span) {                          // (uniform: a span-free clip's backtrace is the plain DP's; skip_b is not null)
                        const int ak = span_first(skip_b, kk >> 1);      // J(kk) = 2 ak, as the sweep computed it
                        if (ak >= 0) {                               // the third mask is meaningful only for states with a span
                            code |= (int)((row[2] >> sh) & 1ull) << 2;
                            if (code >= 3) {                         // labels ak .. kk / 2 - 1 lie inside the taken jump: they stay -1
                                skipped += (kk >> 1) - ak;
                                code = kk - (2 * ak - (code - 3));
                            }
                        }
                    }
                }
                knew = kk - code;
                if ((kk & 1) && knew != kk) on_g[kk >> 1] = j;   // frame j is the first one in this state
            }
            knext = kk;
            kk = knew;
        }
        // the path is monotone in k, so every odd state is entered at most once and taken jumps do not overlap:
        // every label visited or inside a taken jump <=> entered + skipped == L
        if constexpr (!REP) p.status[b] = entered + skipped == L ? LA_OK : LA_EINFEASIBLE;   // reference: ValueError from list.index (:183)
    }
    if constexpr (REP) {
        // every label visited at least once, or inside a taken skip jump (its mark is written out as -1); by the whole workgroup
        __threadfence_block();
        __syncthreads();
        bool missing = false;
        for (int n = tid; n < L; n += NT) {
            const int v = on_g[n];
            if (v == kSkipped) on_g[n] = -1;
            else missing |= v < 0;
        }
        const bool any_missing = __syncthreads_or(missing) != 0;
        if (tid == 0) p.status[b] = any_missing ? LA_EINFEASIBLE : LA_OK;
    }
}

struct VitPlan {
    int strip;   // 0: one lane per state (<= 1024 states); else R = states per thread of the 1024-thread strip kernel
    int nw;
    bool bt_in_lds;
    size_t lds_bytes;
    size_t ws_bytes;
};

// mask_words: 2, or 3 with spans (then the lane-per-state forms also keep J in LDS).  label_limit: 511 = one lane per state only,
// 4095 = the strip kernel beyond that (R = 8 holds 8192 states).  false: more labels than the limit
bool plan_viterbi(int batch, int max_frames, int max_labels, int mask_words, int label_limit, VitPlan *pl) {
    Tile tile;
    if (!plan_tile(max_labels, label_limit, &tile)) return false;
    const int nw = tile.nw;
    pl->strip = 0;
    if (tile.r > 1) {
        const int R = tile.r;
        pl->strip = R;
        pl->nw = 16;
        pl->bt_in_lds = false;
        pl->lds_bytes = 2 * (size_t)(1024 * R + 2) * sizeof(double);
        pl->ws_bytes = (size_t)batch * max_frames * R * 16 * mask_words * sizeof(unsigned long long);
        return true;
    }
    const size_t fixed = 2 * (size_t)(nw * 64 + 2) * sizeof(double) + 2 * (size_t)((max_labels + 3) & ~3) * sizeof(int32_t) +
                         (mask_words == 3 ? (size_t)nw * 64 * sizeof(int32_t) : 0);
    const size_t fixed_al = (fixed + 15) & ~(size_t)15;
    const size_t bt_bytes = (size_t)max_frames * nw * mask_words * sizeof(unsigned long long);
    pl->nw = nw;
    pl->bt_in_lds = fixed_al + bt_bytes <= kLdsBudget;
    pl->lds_bytes = pl->bt_in_lds ? fixed_al + bt_bytes : fixed_al;
    pl->ws_bytes = pl->bt_in_lds ? 0 : (size_t)batch * bt_bytes;
    return true;
}

// the lane-per-state forms; the single wave takes its neighbours by DPP unless the option is off or dp / bt are dumped
template <bool SPANS, bool DUMP, bool WIN = false, bool REP = false>
int launch_lanes(const char *timer, const VitParams &p, const VitPlan &pl, int batch, hipStream_t stream) {
    switch (pl.nw) {
        case 1:
            if (!DUMP && la::opts().viterbi_dpp) return launch<viterbi_kernel<1, true, SPANS, false, WIN, REP>>(timer, 64, p, pl, batch, stream);
            return launch<viterbi_kernel<1, false, SPANS, DUMP, WIN, REP>>(timer, 64, p, pl, batch, stream);
        case 2: return launch<viterbi_kernel<2, false, SPANS, DUMP, WIN, REP>>(timer, 128, p, pl, batch, stream);
        case 4: return launch<viterbi_kernel<4, false, SPANS, DUMP, WIN, REP>>(timer, 256, p, pl, batch, stream);
        case 8: return launch<viterbi_kernel<8, false, SPANS, DUMP, WIN, REP>>(timer, 512, p, pl, batch, stream);
        case 16: return launch<viterbi_kernel<16, false, SPANS, DUMP, WIN, REP>>(timer, 1024, p, pl, batch, stream);
    }
    return LA_EUNSUPPORTED;
}

// the strip forms, R states per thread
template <bool SPANS, bool WIN, bool REP = false>
int launch_strip(const char *timer, const VitParams &p, const VitPlan &pl, int batch, hipStream_t stream) {
    switch (pl.strip) {
        case 2: return launch<viterbi_strip_kernel<2, SPANS, WIN, REP>>(timer, 1024, p, pl, batch, stream);
        case 4: return launch<viterbi_strip_kernel<4, SPANS, WIN, REP>>(timer, 1024, p, pl, batch, stream);
        case 8: return launch<viterbi_strip_kernel<8, SPANS, WIN, REP>>(timer, 1024, p, pl, batch, stream);
    }
    return LA_EUNSUPPORTED;
}

template <bool SPANS, bool WIN, bool REP = false>
int launch_face(const char *timer, const VitParams &p, const VitPlan &pl, int batch, hipStream_t stream) {
    return pl.strip ? launch_strip<SPANS, WIN, REP>(timer, p, pl, batch, stream) : launch_lanes<SPANS, false, WIN, REP>(timer, p, pl, batch, stream);
}

// What the four batch entries (and their workspace queries) differ in.  la_viterbi_lattice_batch takes its face from the pointers that
// are present and answers every argument error under its own name; its workspace is the span planner's (three mask words) whatever
// the face.  Up to 511 labels, and for the plain lattice at any size, its call then IS the matching entry's: that entry's plan (whose
// need is never larger: fewer mask words) and timer; above that the strip kernel's span / window faces under its own timer.
struct Entry {
    FaceNames names;
    int mask_words, label_limit;
    bool limit_first;                      // the label limit is reported before the stride check (la_viterbi_batch: after it)
    const char *over_batch, *over_query;   // the label-limit message of the batch call and of the workspace query
};
// the first three are (int)Face of the entry's fixed face; kLattice, kRepeats: decided per call
enum EntryId { kPlain, kSpans, kWindows, kLattice, kRepeats };
static_assert(kPlain == (int)Face::Plain && kSpans == (int)Face::Spans && kWindows == (int)Face::Windows, "kEntries rows follow Face");
const Entry kEntries[5] = {
    {face_names(Sweep::Dp, Face::Plain), 2, 4095, false, "viterbi: max_labels %d exceeds 4095",
     "viterbi: max_labels %d exceeds 4095 (8192 lattice states per workgroup)"},
    {face_names(Sweep::Dp, Face::Spans), 3, 511, true, "viterbi_spans: max_labels %d exceeds 511 (one lane per lattice state)",
     "viterbi_spans: max_labels %d exceeds 511 (one lane per lattice state)"},
    {face_names(Sweep::Dp, Face::Windows), 3, 511, true, "viterbi_windows: max_labels %d exceeds 511 (one lane per lattice state)",
     "viterbi_windows: max_labels %d exceeds 511 (one lane per lattice state)"},
    {{"viterbi_lattice_batch", "viterbi_lattice", "viterbi_lattice"}, 3, 4095, true,
     "viterbi_lattice: max_labels %d exceeds 4095 (8192 lattice states per workgroup)",
     "viterbi_lattice: max_labels %d exceeds 4095 (8192 lattice states per workgroup)"},
    {{"viterbi_repeats_batch", "viterbi_repeats", "viterbi_repeats"}, 3, 4095, true,
     "viterbi_repeats: max_labels %d exceeds 4095 (8192 lattice states per workgroup)",
     "viterbi_repeats: max_labels %d exceeds 4095 (8192 lattice states per workgroup)"}};

int query_workspace(EntryId id, int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    const Entry &e = kEntries[id];
    LA_CHECK_ARG(bytes && batch >= 0 && max_frames > 0 && max_labels > 0, "%s_workspace_bytes: bad arguments", e.names.query);
    VitPlan pl;
    if (!plan_viterbi(batch, max_frames, max_labels, e.mask_words, e.label_limit, &pl)) {
        la::set_error(e.over_query, max_labels);
        return LA_EUNSUPPORTED;
    }
    *bytes = pl.ws_bytes;
    return LA_OK;
}

// the caller's arguments of a batch entry; null / zero stands in for what the entry does not have
VitParams batch_params(const float *em, int64_t em_batch_stride, int64_t em_row_stride, const int32_t *labels, int32_t labels_stride,
                       const int32_t *n_labels, const int32_t *n_frames, int32_t max_frames, int32_t max_labels, int32_t *onset,
                       int32_t *offset, int32_t out_stride, double *final_score, int32_t *status, const int32_t *skip_from,
                       int32_t skip_stride, double skip_penalty, const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride) {
    VitParams p{};
    p.set_inputs(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels);
    p.set_spans(skip_from, skip_stride, skip_penalty);
    p.set_windows(win_lo, win_hi, win_stride);
    p.set_outputs(onset, offset, out_stride, final_score, status);
    return p;
}

// the four la_viterbi*_batch entry points: p holds the caller's arguments, the workspace fields are set here
int run_batch(EntryId id, VitParams p, int32_t batch, void *workspace, size_t workspace_bytes, hipStream_t stream) {
    const Entry &e = kEntries[id];
    const char *who = e.names.entry;
    if (batch == 0) return LA_OK;
    Face face = id >= kLattice ? Face::Plain : (Face)id;
    if (id == kLattice || id == kRepeats) {
        LA_CHECK_ARG((p.win_lo == nullptr) == (p.win_hi == nullptr), "%s: win_lo and win_hi go together (both null: no windows)", who);
        face = p.win_lo ? Face::Windows : p.skip_from ? Face::Spans : Face::Plain;
    }
    LA_CHECK_ARG(p.inputs_present(face) && p.onset && p.offset && p.final_score && p.status, "%s: null pointer", who);
    LA_CHECK_ARG(p.sizes_ok(batch), "%s: bad sizes", who);
    // (la_viterbi_batch has no penalty: 0.  The lattice entry checks the one it was given whatever the face)
    LA_CHECK_ARG(p.penalty >= 0.0, "%s: skip_penalty must be >= 0 (and not NaN)", who);
    if (id == kRepeats) LA_CHECK_ARG(p.repeat_penalty >= 0.0, "%s: repeat_penalty must be >= 0 (and not NaN)", who);
    VitPlan pl;
    const bool planned = plan_viterbi(batch, p.max_frames, p.max_labels, e.mask_words, e.label_limit, &pl);
    LA_CHECK_ARG(p.strides_ok(face, p.out_stride, false) || (e.limit_first && !planned), "%s: strides smaller than max_labels", who);
    if (!planned) {
        la::set_error(e.over_batch, p.max_labels);
        return LA_EUNSUPPORTED;
    }
    if (id == kRepeats) {
        LA_CHECK_ARG(!p.repeat_from || p.repeat_stride >= p.max_labels, "%s: repeat_stride smaller than max_labels", who);
        LA_CHECK_ARG(!p.path || p.path_stride >= p.max_frames, "%s: path_stride smaller than max_frames", who);
    }
    LA_CHECK_ARG(pl.ws_bytes == 0 || (workspace && workspace_bytes >= pl.ws_bytes), "%s: workspace too small (%zu < %zu)", who,
                 workspace_bytes, pl.ws_bytes);
    LA_CHECK_ARG(pl.ws_bytes == 0 || (uintptr_t)workspace % 8 == 0, "%s: workspace must be 8-byte aligned", who);
    const char *timer = e.names.timer;
    if (id == kLattice && (face == Face::Plain || !pl.strip)) {
        const Entry &own = kEntries[(int)face];
        plan_viterbi(batch, p.max_frames, p.max_labels, own.mask_words, own.label_limit, &pl);
        timer = own.names.timer;
    }
    p.bt_global = reinterpret_cast<unsigned long long *>(workspace);
    p.bt_in_lds = pl.bt_in_lds ? 1 : 0;
    // the repeat face sits on top of the span + window one whatever is given: null pointers are "absent" inside the kernel
    if (id == kRepeats) return launch_face<true, true, true>(timer, p, pl, batch, stream);
    switch (face) {
        case Face::Plain: return launch_face<false, false>(timer, p, pl, batch, stream);
        case Face::Spans: return launch_face<true, false>(timer, p, pl, batch, stream);
        case Face::Windows: return launch_face<true, true>(timer, p, pl, batch, stream);
    }
    return LA_EUNSUPPORTED;
}

}  // namespace

extern "C" int la_viterbi_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    return query_workspace(kPlain, batch, max_frames, max_labels, bytes);
}

extern "C" int la_viterbi_spans_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    return query_workspace(kSpans, batch, max_frames, max_labels, bytes);
}

extern "C" int la_viterbi_windows_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    return query_workspace(kWindows, batch, max_frames, max_labels, bytes);
}

extern "C" int la_viterbi_lattice_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    return query_workspace(kLattice, batch, max_frames, max_labels, bytes);
}

extern "C" int la_viterbi_batch(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                                const int32_t *labels, int32_t labels_stride, const int32_t *n_labels,
                                const int32_t *n_frames, int32_t batch, int32_t max_frames, int32_t max_labels,
                                int32_t *onset, int32_t *offset, int32_t out_stride, double *final_score,
                                int32_t *status, void *workspace, size_t workspace_bytes, void *stream_) {
    return run_batch(kPlain,
                     batch_params(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels, onset,
                                  offset, out_stride, final_score, status, nullptr, 0, 0.0, nullptr, nullptr, 0),
                     batch, workspace, workspace_bytes, (hipStream_t)stream_);
}

extern "C" int la_viterbi_spans_batch(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                                      const int32_t *labels, int32_t labels_stride, const int32_t *n_labels,
                                      const int32_t *n_frames, int32_t batch, int32_t max_frames, int32_t max_labels,
                                      int32_t *onset, int32_t *offset, int32_t out_stride, double *final_score,
                                      int32_t *status, const int32_t *skip_from, int32_t skip_stride, double skip_penalty,
                                      void *workspace, size_t workspace_bytes, void *stream_) {
    return run_batch(kSpans,
                     batch_params(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels, onset,
                                  offset, out_stride, final_score, status, skip_from, skip_stride, skip_penalty, nullptr, nullptr, 0),
                     batch, workspace, workspace_bytes, (hipStream_t)stream_);
}

extern "C" int la_viterbi_windows_batch(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                                        const int32_t *labels, int32_t labels_stride, const int32_t *n_labels,
                                        const int32_t *n_frames, int32_t batch, int32_t max_frames, int32_t max_labels,
                                        int32_t *onset, int32_t *offset, int32_t out_stride, double *final_score,
                                        int32_t *status, const int32_t *skip_from, int32_t skip_stride, double skip_penalty,
                                        const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride,
                                        void *workspace, size_t workspace_bytes, void *stream_) {
    return run_batch(kWindows,
                     batch_params(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels, onset,
                                  offset, out_stride, final_score, status, skip_from, skip_stride, skip_penalty, win_lo, win_hi, win_stride),
                     batch, workspace, workspace_bytes, (hipStream_t)stream_);
}

extern "C" int la_viterbi_lattice_batch(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                                        const int32_t *labels, int32_t labels_stride, const int32_t *n_labels,
                                        const int32_t *n_frames, int32_t batch, int32_t max_frames, int32_t max_labels,
                                        int32_t *onset, int32_t *offset, int32_t out_stride, double *final_score,
                                        int32_t *status, const int32_t *skip_from, int32_t skip_stride, double skip_penalty,
                                        const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride,
                                        void *workspace, size_t workspace_bytes, void *stream_) {
    return run_batch(kLattice,
                     batch_params(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels, onset,
                                  offset, out_stride, final_score, status, skip_from, skip_stride, skip_penalty, win_lo, win_hi, win_stride),
                     batch, workspace, workspace_bytes, (hipStream_t)stream_);
}

extern "C" int la_viterbi_repeats_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes) {
    return query_workspace(kRepeats, batch, max_frames, max_labels, bytes);
}

extern "C" int la_viterbi_repeats_batch(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                                        const int32_t *labels, int32_t labels_stride, const int32_t *n_labels,
                                        const int32_t *n_frames, int32_t batch, int32_t max_frames, int32_t max_labels,
                                        int32_t *onset, int32_t *offset, int32_t out_stride, double *final_score,
                                        int32_t *status, const int32_t *skip_from, int32_t skip_stride, double skip_penalty,
                                        const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride,
                                        const int32_t *repeat_from, int32_t repeat_stride, double repeat_penalty,
                                        int32_t *path, int32_t path_stride,
                                        void *workspace, size_t workspace_bytes, void *stream_) {
    VitParams p = batch_params(em, em_batch_stride, em_row_stride, labels, labels_stride, n_labels, n_frames, max_frames, max_labels, onset,
                               offset, out_stride, final_score, status, skip_from, skip_stride, skip_penalty, win_lo, win_hi, win_stride);
    p.repeat_from = repeat_from, p.repeat_stride = repeat_stride, p.repeat_penalty = repeat_penalty;
    p.path = path, p.path_stride = path_stride;
    return run_batch(kRepeats, p, batch, workspace, workspace_bytes, (hipStream_t)stream_);
}

// run_viterbi_core(dp, bt, lp, ls, label) of the reference (utils/alignment.py:73-119) for ONE utterance: same
// kernel, instantiated so that it also writes every dp row (float64) and backpointer (int64 predecessor state).
extern "C" int la_viterbi_core(const float *em, int64_t em_row_stride, const int32_t *labels, int32_t n_labels_host,
                               int32_t n_frames_host, const int32_t *n_labels, const int32_t *n_frames, double *dp,
                               long long *bt, int32_t *scratch_i32, double *scratch_f64, void *workspace,
                               size_t workspace_bytes, void *stream_) {
    LA_CHECK_ARG(em && labels && n_labels && n_frames && dp && bt && scratch_i32 && scratch_f64, "viterbi_core: null pointer");
    LA_CHECK_ARG(n_labels_host > 0 && n_frames_host > 0 && em_row_stride >= n_labels_host + 1, "viterbi_core: bad sizes");
    VitPlan pl;
    if (!plan_viterbi(1, n_frames_host, n_labels_host, 2, 511, &pl)) {
        la::set_error("viterbi_core: more than 511 labels (the dp / bt dump face is one lane per state)");
        return LA_EUNSUPPORTED;
    }
    LA_CHECK_ARG(pl.ws_bytes == 0 || (workspace && workspace_bytes >= pl.ws_bytes), "viterbi_core: workspace too small");
    VitParams p{};
    p.set_inputs(em, 0, em_row_stride, labels, n_labels_host, n_labels, n_frames, n_frames_host, n_labels_host);
    // scratch_i32: onset[L] | offset[L] | status[1]
    p.set_outputs(scratch_i32, scratch_i32 + n_labels_host, n_labels_host, scratch_f64, scratch_i32 + 2 * n_labels_host);
    p.bt_global = reinterpret_cast<unsigned long long *>(workspace);
    p.bt_in_lds = pl.bt_in_lds ? 1 : 0;
    p.dp_dump = dp;
    p.bt_dump = bt;
    return launch_lanes<false, true>(face_names(Sweep::Dp, Face::Plain).timer, p, pl, 1, (hipStream_t)stream_);
}
