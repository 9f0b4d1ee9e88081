"""tests/windows_reference.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The alignment DP with per-state frame windows (include/lyricalign.h la_viterbi_windows_batch) as plain Python float64: state s of
the S = 2L+1 lattice states (0 = leading silence, 2n+1 = label n, 2n+2 = the silence after it) may hold the path at frame t only
if lo[s] <= t < hi[s].  dp[t][s] is computed by the rule of tests/optional_spans_reference.py (whose jump arcs are imported, not
restated) and then set to -inf when the cell lies outside its window, row 0 included.  The yardstick of tests/test_gpu_windows.py
(equality to the bit) and itself pinned by tests/test_host_windows.py against optional_spans_reference.viterbi_spans (open
windows), oracle/viterbi_python.py (open windows, no spans) and exhaustive enumeration of the lattice paths inside the windows.
"""
from __future__ import annotations

import numpy as np

import optional_spans_reference as osr
from optional_spans_reference import LA_EEMPTY, LA_EINFEASIBLE, LA_EINVAL, LA_OK, NEG  # noqa: F401  (re-exported for the tests)

NINF = float("-inf")


def open_windows(L, T):
    """-> (lo, hi) of 2L+1 entries that allow every state at every frame of a T-frame clip."""
    return [0] * (2 * L + 1), [int(T)] * (2 * L + 1)


def lattice(em, labels, lo, hi, skip_from=None, penalty=0.0):
    """em [T][>= L+1] (float32 values) -> dp [T][S] (float64, -inf outside the windows), bt [T][S] (predecessor state),
    jumped [T][S] (the predecessor was reached over a span's arc).  skip_from None = no span anywhere."""
    L = len(labels)
    S = 2 * L + 1
    T = len(em)
    penalty = float(penalty)
    if skip_from is None:
        skip_from = [-1] * (L + 1)
    J, jm1 = osr.jump_sources(labels, skip_from)
    may_skip = [s % 2 == 1 and s >= 3 and labels[s // 2] != labels[s // 2 - 1] for s in range(S)]
    col = [1 + s // 2 if s % 2 else 0 for s in range(S)]
    rows = [[float(v) for v in em[t][: L + 1]] for t in range(T)]

    def inside(t, s):
        return int(lo[s]) <= t < int(hi[s])

    prev = [NEG] * S
    prev[0] = rows[0][0]
    prev[1] = rows[0][1]
    prev = [v if inside(0, s) else NINF for s, v in enumerate(prev)]
    dp, bt, jumped = [prev], [[0] * S], [[False] * S]
    for t in range(1, T):
        e = rows[t]
        cur, src_row, jump_row = [0.0] * S, [0] * S, [False] * S
        cur[0] = (prev[0] + e[0]) if inside(t, 0) else NINF
        for s in range(1, S):
            p0, p1 = prev[s], prev[s - 1]
            if may_skip[s] and prev[s - 2] >= p1 and prev[s - 2] >= p0:
                best, src = prev[s - 2], s - 2
            elif p0 > p1:
                best, src = p0, s
            else:
                best, src = p1, s - 1
            j, jump = J[s], False
            if j >= 0:
                v = prev[j] - penalty
                if v > best:
                    best, src, jump = v, j, True
                if jm1[s]:
                    v = prev[j - 1] - penalty
                    if v > best:
                        best, src, jump = v, j - 1, True
            cur[s] = (best + e[col[s]]) if inside(t, s) else NINF
            src_row[s] = src
            jump_row[s] = jump
        dp.append(cur)
        bt.append(src_row)
        jumped.append(jump_row)
        prev = cur
    return dp, bt, jumped


def lattice_rows(em, labels, lo, hi, skip_from=None, penalty=0.0):
    """lattice() with each row's states updated together as numpy float64 vectors: the same IEEE adds, subtracts and comparisons in the
    same order per cell, so dp / bt / jumped are lattice()'s cell by cell (tests/test_host_windows.py pins that); for the lattices of
    hundreds of states that tests/test_gpu_windows.py compares the kernel with.  -> numpy arrays."""
    L = len(labels)
    S = 2 * L + 1
    T = len(em)
    penalty = float(penalty)
    if skip_from is None:
        skip_from = [-1] * (L + 1)
    J, jm1 = osr.jump_sources(labels, skip_from)
    J, jm1 = np.asarray(J), np.asarray(jm1, dtype=bool)
    has_j = J >= 0
    j_src, jm1_src = np.where(has_j, J, 0), np.where(jm1, J - 1, 0)
    may_skip = np.asarray([s % 2 == 1 and s >= 3 and labels[s // 2] != labels[s // 2 - 1] for s in range(S)], dtype=bool)
    col = np.asarray([1 + s // 2 if s % 2 else 0 for s in range(S)])
    rows = np.asarray(em, dtype=np.float32)[:, : L + 1].astype(np.float64)
    lo, hi = np.asarray(lo[:S], dtype=np.int64), np.asarray(hi[:S], dtype=np.int64)
    states = np.arange(S)
    dp = np.empty((T, S), dtype=np.float64)
    bt = np.zeros((T, S), dtype=np.int64)
    jumped = np.zeros((T, S), dtype=bool)
    prev = np.full((S,), NEG)
    prev[0], prev[1] = rows[0, 0], rows[0, 1]
    prev[~((lo <= 0) & (0 < hi))] = NINF
    dp[0] = prev
    for t in range(1, T):
        p0 = prev
        p1 = np.concatenate([[NEG], prev[:-1]])
        p2 = np.concatenate([[NEG, NEG], prev[:-2]])
        skip = may_skip & (p2 >= p1) & (p2 >= p0)
        stay = p0 > p1
        best = np.where(skip, p2, np.where(stay, p0, p1))
        src = np.where(skip, states - 2, np.where(stay, states, states - 1))
        best[0], src[0] = p0[0], 0
        v = prev[j_src] - penalty
        m = has_j & (v > best)
        best, src = np.where(m, v, best), np.where(m, J, src)
        v = prev[jm1_src] - penalty
        m2 = jm1 & (v > best)
        best, src = np.where(m2, v, best), np.where(m2, J - 1, src)
        cur = best + rows[t, col]
        cur[~((lo <= t) & (t < hi))] = NINF
        dp[t], bt[t], jumped[t] = cur, src, m | m2
        prev = cur
    return dp, bt, jumped


def viterbi_windows(em, labels, lo, hi, skip_from=None, penalty=0.0, rows=False):
    """-> (onset [L], offset [L], score, status, path).  A winning final score of -inf: LA_EINFEASIBLE, score -inf, every onset and
    offset -1, an empty path.  Otherwise the backtrace and status of optional_spans_reference.viterbi_spans.  rows: fill the lattice with
    lattice_rows (the same cells, faster for wide lattices)."""
    L = len(labels)
    if L == 0:
        return [], [], 0.0, LA_EEMPTY, []
    T = len(em)
    if T <= 0:
        return [-1] * L, [-1] * L, 0.0, LA_EINVAL, []
    S = 2 * L + 1
    labels = [int(v) for v in labels]
    if skip_from is None:
        skip_from = [-1] * (L + 1)
    dp, bt, jumped = (lattice_rows if rows else lattice)(em, labels, lo, hi, skip_from, penalty)
    kk = S - 1 if dp[T - 1][S - 1] > dp[T - 1][S - 2] else S - 2
    score = float(dp[T - 1][kk])
    if score == NINF:
        return [-1] * L, [-1] * L, NINF, LA_EINFEASIBLE, []
    path = [kk]
    skipped = [False] * L
    for t in range(T - 1, 0, -1):
        src = int(bt[t][kk])
        if jumped[t][kk]:
            for m in range(int(skip_from[kk // 2]), kk // 2):
                skipped[m] = True
        kk = src
        path.append(kk)
    path.reverse()
    onset, offset = [-1] * L, [-1] * L
    for t, s in enumerate(path):
        if s % 2 == 1:
            n = s // 2
            if onset[n] < 0:
                onset[n] = t
            offset[n] = t + 1
    status = LA_OK
    for n in range(L):
        if onset[n] < 0 and not skipped[n]:
            status = LA_EINFEASIBLE
    return onset, offset, score, status, path


def enumerate_best(em, labels, lo, hi, skip_from=None, penalty=0.0):
    """Exhaustive search over every lattice path that stays inside the windows (start states 0 / 1, end states S-1 / S-2, the arcs of
    optional_spans_reference.arcs): the best score, accumulated in the DP's order, or None when no such path exists."""
    L = len(labels)
    S = 2 * L + 1
    T = len(em)
    penalty = float(penalty)
    if skip_from is None:
        skip_from = [-1] * (L + 1)
    preds = osr.arcs(labels, skip_from)
    succ = [[] for _ in range(S)]
    for s in range(S):
        for src, jump in preds[s]:
            if s == 0 and src != 0:
                continue
            succ[src].append((s, jump))
    col = [1 + s // 2 if s % 2 else 0 for s in range(S)]
    best = [None]

    def inside(t, s):
        return int(lo[s]) <= t < int(hi[s])

    def walk(t, s, score):
        if t == T - 1:
            if s in (S - 1, S - 2) and (best[0] is None or score > best[0]):
                best[0] = score
            return
        for nxt, jump in succ[s]:
            if not inside(t + 1, nxt):
                continue
            v = score - penalty if jump else score
            walk(t + 1, nxt, v + float(em[t + 1][col[nxt]]))

    for s0 in (0, 1):
        if inside(0, s0):
            walk(0, s0, float(em[0][col[s0]]))
    return best[0]
