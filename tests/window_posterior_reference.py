"""CPU yardstick of the alignment posteriors on the lattice with per-state frame windows (helper, not collected as a test): the float64
numpy forward-backward of tests/span_posterior_reference.py -- its arcs (spr.arc_arrays), its emission gather and its log-sum-exp are
imported, not restated -- with the emission matrix set to -inf outside the windows, and a brute-force enumerator of the paths inside the
windows for lattices small enough to enumerate.  Definitions: include/lyricalign.h, la_alignment_posteriors_windows.

A cell (t, s) weighs zero unless lo[s] <= t < hi[s]: the sums (alpha, beta, the entry / exit / span-skip terms) use the masked emission.
gamma = exp(alpha + beta - e - log_z) subtracts the UNMASKED emission: alpha and beta are already -inf outside the window, where the
masked value would give -inf - (-inf).  log_z is the windowed one, so every output is a posterior GIVEN the windows.
"""
import numpy as np

import optional_spans_reference as osr
import posterior_reference as pr
import span_posterior_reference as spr

NEG = -np.inf


def inside(T, S, lo, hi):
    """-> bool [T,S]: cell (t, s) lies inside its window."""
    t = np.arange(T)[:, None]
    return (t >= np.asarray(lo[:S], np.int64)[None]) & (t < np.asarray(hi[:S], np.int64)[None])


def posteriors(em, labels, lo, hi, skip_from=None, penalty=0.0):
    """em [T, >= L+1] compact float32, lo / hi [>= 2L+1] ints -> gamma [T,S], entry [T,L], exit [T,L], present [L], span_skip [L+1], log_z
    as spr.posteriors, on the paths inside the windows.  skip_from None: no span anywhere.  All zero (log_z = -inf) when no path exists."""
    labels = [int(v) for v in labels]
    L = len(labels)
    S = 2 * L + 1
    T = np.asarray(em).shape[0]
    penalty = float(penalty)
    skip_from = [-1] * (L + 1) if skip_from is None else skip_from
    e = spr._emissions(em, L)
    eg = np.where(inside(T, S, lo, hi), e, NEG)
    src, dst, jump = spr.arc_arrays(labels, skip_from)
    cost = np.where(jump, penalty, 0.0)
    other = src != dst
    alpha = np.full((T, S), NEG)
    alpha[0, 0] = eg[0, 0]
    alpha[0, 1] = eg[0, 1]
    inc = np.full((T, S), NEG)
    for t in range(1, T):
        vals = alpha[t - 1, src] - cost
        alpha[t] = spr._lse_at(S, dst, vals) + eg[t]
        inc[t] = spr._lse_at(S, dst[other], vals[other])
    beta = np.full((T, S), NEG)
    beta[T - 1, S - 1] = eg[T - 1, S - 1]
    beta[T - 1, S - 2] = eg[T - 1, S - 2]
    out = np.full((T, S), NEG)
    for t in range(T - 2, -1, -1):
        vals = beta[t + 1, dst] - cost
        beta[t] = spr._lse_at(S, src, vals) + eg[t]
        out[t] = spr._lse_at(S, src[other], vals[other])
    log_z = np.logaddexp(alpha[T - 1, S - 1], alpha[T - 1, S - 2])
    if np.isneginf(log_z):
        return np.zeros((T, S)), np.zeros((T, L)), np.zeros((T, L)), np.zeros(L), np.zeros(L + 1), log_z
    odd = np.arange(1, S, 2)
    with np.errstate(invalid="ignore"):
        gamma = pr._exp0(alpha + beta - e - log_z)                 # the unmasked emission; alpha = beta = -inf outside: 0
        entry = pr._exp0(inc[:, odd] + beta[:, odd] - log_z)
        exit_ = pr._exp0(alpha[:, odd] + out[:, odd] - log_z)
        entry[0] = gamma[0, odd]
        exit_[T - 1] = gamma[T - 1, odd]
        span_skip = np.zeros(L + 1)
        if T > 1 and jump.any():
            js, jd = src[jump], dst[jump]
            mass = pr._exp0(alpha[:-1][:, js] - penalty + beta[1:][:, jd] - log_z).sum(0)
            np.add.at(span_skip, jd // 2, mass)
    return gamma, entry, exit_, entry.sum(0), span_skip, log_z


def brute(em, labels, lo, hi, skip_from=None, penalty=0.0):
    """All paths of a small lattice that stay inside the windows -> gamma [T,S], log_z, present [L], span_skip [L+1]; None when there is
    no such path."""
    labels = [int(v) for v in labels]
    L = len(labels)
    S = 2 * L + 1
    T = np.asarray(em).shape[0]
    penalty = float(penalty)
    skip_from = [-1] * (L + 1) if skip_from is None else skip_from
    e = spr._emissions(em, L)
    ok = inside(T, S, lo, hi)
    succ = [[] for _ in range(S)]
    for s, plist in enumerate(osr.arcs(labels, skip_from)):
        for a, j in plist:
            succ[a].append((s, j))
    occ = np.zeros((T, S))
    present = np.zeros(L)
    skip = np.zeros(L + 1)
    z = [0.0]

    def walk(path, score, jumps):
        t = len(path)
        if t == T:
            if path[-1] >= S - 2:
                w = np.exp(score)
                z[0] += w
                for tt, s in enumerate(path):
                    occ[tt, s] += w
                for n in {s // 2 for s in path if s % 2}:
                    present[n] += w
                for n in jumps:
                    skip[n] += w
            return
        for nxt, j in succ[path[-1]]:
            if ok[t, nxt]:
                walk(path + [nxt], score - (penalty if j else 0.0) + e[t, nxt], jumps + [nxt // 2] if j else jumps)

    for s0 in (0, 1):
        if s0 < S and ok[0, s0]:
            walk([s0], e[0, s0], [])
    if z[0] == 0.0:
        return None
    return occ / z[0], np.log(z[0]), present / z[0], skip / z[0]


# The inputs of tests/test_gpu_window_posteriors.py's shape cases, built as tests/test_gpu_windows.py builds the DP's: per shape three
# lattices (no spans with a null skip_from, two optional lines at penalty 0 and at penalty 1), two clips each; clip 0 has its windows
# around its own best path, clip 1 around the best path of a second emission draw (widened by 0..3 frames per side), so its windows bind.
# tests/test_host_window_posteriors.py asserts on the CPU that every window set has a path and moves gamma by more than 0.5 somewhere --
# otherwise the device test would be vacuous.
# 511 labels do not fit into 300 frames unless lines are left out: at (300, 511) the span-free lattice has no path under any windows.  It
# stays in as a case where kernel and yardstick must agree on LA_EINFEASIBLE (open windows), and the span-free lattice of 511 labels is
# checked at 600 frames instead -- (600, 511) holds that lattice alone.
GPU_SHAPES = [(40, 5), (90, 31), (100, 32), (300, 100), (450, 200), (400, 300), (300, 511), (600, 511)]
_CASES = {}


def gpu_cases(T, L):
    """-> [(skip_from or None, penalty, labels, [em0, em1], [lo0, lo1], [hi0, hi1], [ref0, ref1], feasible)], ref = posteriors(...) of the
    clip; computed once per shape and shared (the entries are not to be modified)."""
    if (T, L) in _CASES:
        return _CASES[(T, L)]
    import test_gpu_windows as tgw
    import windows_reference as wr
    lab = tgw._labels(7 * T + L, L)
    S = 2 * L + 1
    out = []
    for v, (skip, pen) in enumerate([(None, 0.0), (tgw._two_optional_lines(L), 0.0), (tgw._two_optional_lines(L), 1.0)]):
        if (T, L) == (600, 511) and v > 0:
            continue
        rs = np.random.RandomState(1000 * v + 31 * T + L)
        ems = [tgw._emissions(100 + v, T, lab, 0.0), tgw._emissions(200 + v, T, lab, 1.5)]
        other = tgw._emissions(300 + v, T, lab, 1.5 * (v % 2))
        feasible = skip is not None or T >= L
        los, his, refs = [], [], []
        for c, em in enumerate(ems):
            lo, hi = wr.open_windows(L, T)
            if feasible:
                base = wr.viterbi_windows(em if c == 0 else other, lab, lo, hi, skip, pen, rows=True)
                assert base[3] == wr.LA_OK, (T, L, v, c)
                lo, hi = tgw._windows_around(rs, base[4], S, T)
            los.append(lo); his.append(hi)
            refs.append(posteriors(em, lab, lo, hi, skip, pen))
        out.append((skip, pen, lab, ems, los, his, refs, feasible))
    _CASES[(T, L)] = out
    return out


# The prefetch edges of tests/test_gpu_window_posteriors.py: T around the block depths (8 frames in the one-wave forms, 4 in the multi-wave
# forms, 2 / 1 with spans) at the smallest lattices and at the first two-wave size.
EDGE_SHAPES = [(T, L) for L in (1, 2) for T in (1, 2, 8, 9, 10, 17)] + [(T, 32) for T in (66, 67, 68, 69)]


def edge_cases(T, L):
    """-> [(skip_from or None, penalty, labels, em, lo, hi, ref, feasible)] without spans and with (L = 1: its only span; else two optional
    lines, penalty 0.5).  The windows stay open except that two states of the open-window DP's path (the one it holds at frame T // 2
    and its last one) are narrowed to their segment of that path, so the path stays inside.  T = 1 at L = 2 has no path in any lattice:
    open windows, kernel and yardstick must agree on LA_EINFEASIBLE."""
    if ("edge", T, L) in _CASES:
        return _CASES[("edge", T, L)]
    import test_gpu_windows as tgw
    import windows_reference as wr
    lab = tgw._labels(11 * T + L, L)
    out = []
    for v, (skip, pen) in enumerate([(None, 0.0), ([-1, 0] if L == 1 else tgw._two_optional_lines(L), 0.5)]):
        em = tgw._emissions(400 + v + T, T, lab, 1.0 * v)
        lo, hi = wr.open_windows(L, T)
        base = wr.viterbi_windows(em, lab, lo, hi, skip, pen, rows=True)
        feasible = base[3] == wr.LA_OK
        assert feasible == (not (T == 1 and L >= 2)), (T, L, v)
        if feasible:
            path = list(base[4])
            for s in {path[T // 2], path[-1]}:
                lo[s], hi[s] = path.index(s), T - path[::-1].index(s)
        out.append((skip, pen, lab, em, lo, hi, posteriors(em, lab, lo, hi, skip, pen), feasible))
    _CASES[("edge", T, L)] = out
    return out
