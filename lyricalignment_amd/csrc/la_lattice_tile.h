// la_lattice_tile.h -- THE TILE FORM of a kernel that sweeps the alignment lattice frame by frame, and the host path of its entry.
//
// One workgroup per clip, NW * 64 threads, thread tid owns the R consecutive states tid * R + r of the S = 2L+1 (0 = leading silence,
// 2n+1 = label n, 2n+2 = the silence after it).  R = 1 with NW = waves_for_labels(L) up to 511 labels; beyond 16 waves 1024 threads
// with R = 2 / 4 / 8 up to 1023 / 2047 / 4095 labels: eight forms (NW, R) in all.  Per frame the k-1 / k-2 neighbours of a thread's
// first states cross threads through a double-buffered f64 row in LDS with ONE barrier (one wave: DPP shifts, no LDS, no barrier);
// emissions are prefetched SPF frames ahead into registers; backpointers are ballot words per (frame, r, wave) in the workspace.
//
// This header holds the recurrence cell and the HOST side of that form: the planner of (NW, R), the launch, the dispatcher over the eight
// forms and the tail of an entry's argument checks.  The planner and the launch also serve la_viterbi.hip and la_posterior.hip, whose
// kernels keep their own mapping.  The kernels of la_line_order.hip, la_line_posterior.hip and la_min_duration.hip keep the device side
// of the form in their own text: written through shared device helpers (owned state, prologue, neighbour exchange, frame loop, masks)
// the two DPs gave the parent's bits but several forms ran 1 - 5 % slower (profiles/lattice_tile_refactor.txt, section 3).
#pragma once

#include <type_traits>

#include "la_lattice.h"

namespace la {
namespace lattice {

constexpr double kNeg = -10000000.0;  // utils/alignment.py:144

// ---- the recurrence cell: the winner among a state's predecessors and its backpointer code --------------------------------------
struct Cell {
    int code;      // 0 stay, 1 advance, 2 skip: the offset back to the predecessor; 3 and above: a jump, numbered by the kernel that has it
    double best;
};
// p0, p1, p2: dp[j-1][k], [k-1], [k-2]; the reference's comparisons in the reference's order
__device__ __forceinline__ Cell choose_neighbour(double p0, double p1, double p2, bool can_skip, bool state0) {
    const bool stay = p0 > p1;                                   // strict (:85,:94,:110)
    const bool skip = can_skip && (p2 >= p1) && (p2 >= p0);      // (:104-105)
    int code = skip ? 2 : (stay ? 0 : 1);
    double best = skip ? p2 : (stay ? p0 : p1);
    if (state0) { code = 0; best = p0; }                         // (:78-82)
    return {code, best};
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
struct Tile {
    int nw, r;
    int states() const { return nw * 64 * r; }   // the state capacity of the workgroup
};
// false: more labels than label_limit (511 = one lane per state only, 4095 = R = 8 holds 8192 states)
inline bool plan_tile(int max_labels, int label_limit, Tile *t) {
    if (max_labels > label_limit) return false;
    t->nw = waves_for_labels(max_labels), t->r = 1;
    if (t->nw > 16) {
        t->nw = 16;
        t->r = 2;
        while (1024 * t->r < 2 * max_labels + 1) t->r *= 2;
    }
    return true;
}

// One launch of a lattice kernel: Plan has lds_bytes, which never exceeds kLdsBudget.
template <auto Kern, class Params, class Plan>
int launch(const char *timer, int threads, const Params &p, const Plan &pl, int batch, hipStream_t stream) {
    static la::DeviceOnce attr_once;            // once per instantiation, to the planners' budget
    if (pl.lds_bytes > 48 * 1024 && attr_once.pending()) {
        LA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
        attr_once.mark();
    }
    la::TimerScope ts(timer, stream);
    hipLaunchKernelGGL(Kern, dim3(batch), dim3(threads), pl.lds_bytes, stream, p);
    LA_LAUNCH_CHECK();
    return LA_OK;
}

// the eight forms: f(NW, R) with both as std::integral_constant, so that f can name Kern<nw, r>
template <class F>
int for_tile(const Tile &t, F &&f) {
    using std::integral_constant;
    constexpr integral_constant<int, 1> one{};
    constexpr integral_constant<int, 16> wide{};
    if (t.r == 1) {
        switch (t.nw) {
            case 1: return f(one, one);
            case 2: return f(integral_constant<int, 2>{}, one);
            case 4: return f(integral_constant<int, 4>{}, one);
            case 8: return f(integral_constant<int, 8>{}, one);
            case 16: return f(wide, one);
        }
    }
    switch (t.r) {
        case 2: return f(wide, integral_constant<int, 2>{});
        case 4: return f(wide, integral_constant<int, 4>{});
        case 8: return f(wide, integral_constant<int, 8>{});
    }
    return LA_EUNSUPPORTED;
}

// The tail of a tile entry's argument checks.  over_label_limit: what the planner's `false` is reported as, by the batch call and by
// the workspace query under the query's name.  check_path_and_workspace: after the entry's own stride checks.
inline int over_label_limit(const char *query, int max_labels) {
    la::set_error("%s: max_labels %d exceeds 4095 (8192 lattice states per workgroup)", query, max_labels);
    return LA_EUNSUPPORTED;
}
inline int check_path_and_workspace(const char *who, bool has_path, int32_t path_stride, int32_t max_frames, const void *workspace,
                                    size_t workspace_bytes, size_t need) {
    LA_CHECK_ARG(!has_path || path_stride >= max_frames, "%s: path_stride smaller than max_frames", who);
    LA_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
    LA_CHECK_ARG((uintptr_t)workspace % 8 == 0, "%s: workspace must be 8-byte aligned", who);
    return LA_OK;
}

}  // namespace lattice
}  // namespace la
