"""tests/repeat_spans_reference.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The alignment DP on the lattice with REPEATABLE label spans (include/lyricalign.h la_viterbi_repeats_batch) as plain Python float64:
recurrence, backtrace, first-visit onsets, the visits of a path, status.  The yardstick of tests/test_gpu_repeat_spans.py (equality
to the bit) and itself pinned by tests/test_host_repeat_spans.py against optional_spans_reference.viterbi_spans (no repeat arcs) and
against exhaustive enumeration of the lattice paths (with them).

States: 0 = leading silence, 2n+1 = label n, 2n+2 = the silence after label n; S = 2L+1.  repeat_from[a] = e with a < e <= L makes
labels a .. e-1 repeatable: the odd state 2a+1 may also be entered from K = 2e (always) and from K-1 = 2e-1 (label e-1, only when
labels[a] != labels[e-1]), both from the previous frame.  Any other entry (-1 by convention) is no span and never an index.  Per cell:
the neighbour rule, then the optional span's J and J-1 (optional_spans_reference, imported, not restated), then dp[K] - repeat_penalty
and dp[K-1] - repeat_penalty, each replacing the winner only if STRICTLY greater; the emission is added last and a cell outside its
frame window (lo[s] <= t < hi[s], tests/windows_reference.py) is -inf.  Backpointer codes: 0 stay, 1 advance, 2 skip, 3 from J,
4 from J-1, 5 from K, 6 from K-1.
"""
from __future__ import annotations

import numpy as np

import optional_spans_reference as osr
from optional_spans_reference import LA_EEMPTY, LA_EINFEASIBLE, LA_EINVAL, LA_OK, NEG  # noqa: F401  (re-exported for the tests)

NINF = float("-inf")


def repeat_sources(labels, repeat_from):
    """-> K[s] (2e, or -1 for none), km1[s] (arc from K-1 allowed) for the S = 2L+1 states.  Only odd states carry a K."""
    L = len(labels)
    S = 2 * L + 1
    K, km1 = [-1] * S, [False] * S
    if repeat_from is None:
        return K, km1
    for a in range(L):
        e = int(repeat_from[a])
        if a < e <= L:
            K[2 * a + 1] = 2 * e
            km1[2 * a + 1] = labels[a] != labels[e - 1]
    return K, km1


def arcs(labels, skip_from=None, repeat_from=None):
    """-> preds[s] = list of (source state, kind): kind 0 = the plain lattice's arcs, 1 = an optional span's jump, 2 = a repeat arc."""
    L = len(labels)
    if skip_from is None:
        skip_from = [-1] * (L + 1)
    preds = [[(src, 1 if jump else 0) for src, jump in p] for p in osr.arcs(labels, skip_from)]
    K, km1 = repeat_sources(labels, repeat_from)
    for s in range(2 * L + 1):
        if K[s] >= 0:
            preds[s].append((K[s], 2))
            if km1[s]:
                preds[s].append((K[s] - 1, 2))
    return preds


def _open(lo, hi, S, T):
    return ([0] * S if lo is None else lo), ([int(T)] * S if hi is None else hi)


def lattice(em, labels, skip_from=None, penalty=0.0, repeat_from=None, repeat_penalty=0.0, lo=None, hi=None):
    """em [T][>= L+1] (float32 values) -> dp [T][S] (float64), bt [T][S] (predecessor state), code [T][S] (0 .. 6)."""
    L = len(labels)
    S = 2 * L + 1
    T = len(em)
    penalty, repeat_penalty = float(penalty), float(repeat_penalty)
    if skip_from is None:
        skip_from = [-1] * (L + 1)
    lo, hi = _open(lo, hi, S, T)
    J, jm1 = osr.jump_sources(labels, skip_from)
    K, km1 = repeat_sources(labels, repeat_from)
    may_skip = [s % 2 == 1 and s >= 3 and labels[s // 2] != labels[s // 2 - 1] for s in range(S)]
    col = [1 + s // 2 if s % 2 else 0 for s in range(S)]
    rows = [[float(v) for v in em[t][: L + 1]] for t in range(T)]

    def inside(t, s):
        return int(lo[s]) <= t < int(hi[s])

    prev = [NEG] * S
    prev[0] = rows[0][0]
    prev[1] = rows[0][1]
    prev = [v if inside(0, s) else NINF for s, v in enumerate(prev)]
    dp, bt, codes = [prev], [[0] * S], [[0] * S]
    for t in range(1, T):
        e = rows[t]
        cur, src_row, code_row = [0.0] * S, [0] * S, [0] * S
        for s in range(S):
            p0 = prev[s]
            if s == 0:
                best, src, code = p0, 0, 0
            else:
                p1 = prev[s - 1]
                if may_skip[s] and prev[s - 2] >= p1 and prev[s - 2] >= p0:
                    best, src, code = prev[s - 2], s - 2, 2
                elif p0 > p1:
                    best, src, code = p0, s, 0
                else:
                    best, src, code = p1, s - 1, 1
            j = J[s]
            if j >= 0:
                v = prev[j] - penalty
                if v > best:
                    best, src, code = v, j, 3
                if jm1[s]:
                    v = prev[j - 1] - penalty
                    if v > best:
                        best, src, code = v, j - 1, 4
            k = K[s]
            if k >= 0:
                v = prev[k] - repeat_penalty
                if v > best:
                    best, src, code = v, k, 5
                if km1[s]:
                    v = prev[k - 1] - repeat_penalty
                    if v > best:
                        best, src, code = v, k - 1, 6
            cur[s] = (best + e[col[s]]) if inside(t, s) else NINF
            src_row[s] = src
            code_row[s] = code
        dp.append(cur)
        bt.append(src_row)
        codes.append(code_row)
        prev = cur
    return dp, bt, codes


def lattice_rows(em, labels, skip_from=None, penalty=0.0, repeat_from=None, repeat_penalty=0.0, lo=None, hi=None):
    """lattice() with each row's states updated together as numpy float64 vectors: the same IEEE adds, subtracts and comparisons in the
    same order per cell, so dp / bt / code are lattice()'s cell by cell (tests/test_host_repeat_spans.py pins that).  -> numpy arrays."""
    L = len(labels)
    S = 2 * L + 1
    T = len(em)
    penalty, repeat_penalty = float(penalty), float(repeat_penalty)
    if skip_from is None:
        skip_from = [-1] * (L + 1)
    lo, hi = _open(lo, hi, S, T)
    J, jm1 = osr.jump_sources(labels, skip_from)
    K, km1 = repeat_sources(labels, repeat_from)
    J, jm1, K, km1 = np.asarray(J), np.asarray(jm1, dtype=bool), np.asarray(K), np.asarray(km1, dtype=bool)
    has_j, has_k = J >= 0, K >= 0
    j_src, jm1_src = np.where(has_j, J, 0), np.where(jm1, J - 1, 0)
    k_src, km1_src = np.where(has_k, K, 0), np.where(km1, K - 1, 0)
    may_skip = np.asarray([s % 2 == 1 and s >= 3 and labels[s // 2] != labels[s // 2 - 1] for s in range(S)], dtype=bool)
    col = np.asarray([1 + s // 2 if s % 2 else 0 for s in range(S)])
    rows = np.asarray(em, dtype=np.float32)[:, : L + 1].astype(np.float64)
    lo, hi = np.asarray(lo[:S], dtype=np.int64), np.asarray(hi[:S], dtype=np.int64)
    states = np.arange(S)
    dp = np.empty((T, S), dtype=np.float64)
    bt = np.zeros((T, S), dtype=np.int64)
    codes = np.zeros((T, S), dtype=np.int64)
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
        code = np.where(skip, 2, np.where(stay, 0, 1))
        src = states - code
        best[0], src[0], code[0] = p0[0], 0, 0
        for ok, idx, pen, base, c in ((has_j, j_src, penalty, J, 3), (jm1, jm1_src, penalty, J - 1, 4),
                                      (has_k, k_src, repeat_penalty, K, 5), (km1, km1_src, repeat_penalty, K - 1, 6)):
            v = prev[idx] - pen
            m = ok & (v > best)
            best, src, code = np.where(m, v, best), np.where(m, base, src), np.where(m, c, code)
        cur = best + rows[t, col]
        cur[~((lo <= t) & (t < hi))] = NINF
        dp[t], bt[t], codes[t] = cur, src, code
        prev = cur
    return dp, bt, codes


class Result(tuple):
    """(onset, offset, score, status, path) -- and, for the tests' non-vacuity conditions, how many arcs of each kind the path took."""
    n_jumps = 0
    n_repeats = 0


def segments(path):
    """The visits of a path: the maximal runs of frames in one odd state, in time order -> [(label index, first frame, last frame + 1)]."""
    out = []
    t, T = 0, len(path)
    while t < T:
        s = int(path[t])
        u = t
        while u + 1 < T and int(path[u + 1]) == s:
            u += 1
        if s >= 0 and s % 2 == 1:
            out.append((s // 2, t, u + 1))
        t = u + 1
    return out


def viterbi(em, labels, skip_from=None, penalty=0.0, repeat_from=None, repeat_penalty=0.0, lo=None, hi=None, rows=False):
    """-> Result (onset [L], offset [L], score, status, path).  onset / offset: a label's FIRST visit in time, -1 / -1 for a label never
    visited.  LA_OK iff every label is visited at least once or lies inside a skip jump the path took (a visit on another pass wins: the
    label then has an onset).  A winning final score of -inf (no path inside the windows): LA_EINFEASIBLE, every onset / offset -1, an
    empty path.  rows: fill the lattice with lattice_rows."""
    L = len(labels)
    if L == 0:
        return Result(([], [], 0.0, LA_EEMPTY, []))
    T = len(em)
    if T <= 0:
        return Result(([-1] * L, [-1] * L, 0.0, LA_EINVAL, []))
    S = 2 * L + 1
    labels = [int(v) for v in labels]
    if skip_from is None:
        skip_from = [-1] * (L + 1)
    dp, bt, codes = (lattice_rows if rows else lattice)(em, labels, skip_from, penalty, repeat_from, repeat_penalty, lo, hi)
    kk = S - 1 if dp[T - 1][S - 1] > dp[T - 1][S - 2] else S - 2
    score = float(dp[T - 1][kk])
    if score == NINF:
        return Result(([-1] * L, [-1] * L, NINF, LA_EINFEASIBLE, []))
    path = [kk]
    skipped = [False] * L
    n_jumps = n_repeats = 0
    for t in range(T - 1, 0, -1):
        code = int(codes[t][kk])
        if code in (3, 4):
            n_jumps += 1
            for m in range(int(skip_from[kk // 2]), kk // 2):
                skipped[m] = True
        elif code >= 5:
            n_repeats += 1
        kk = int(bt[t][kk])
        path.append(kk)
    path.reverse()
    onset, offset = [-1] * L, [-1] * L
    for n, first, end in segments(path):
        if onset[n] < 0:
            onset[n], offset[n] = first, end
    status = LA_OK
    for n in range(L):
        if onset[n] < 0 and not skipped[n]:
            status = LA_EINFEASIBLE
    r = Result((onset, offset, score, status, path))
    r.n_jumps, r.n_repeats = n_jumps, n_repeats
    return r


def enumerate_best(em, labels, skip_from=None, penalty=0.0, repeat_from=None, repeat_penalty=0.0, lo=None, hi=None):
    """Exhaustive search over every lattice path inside the windows (start states 0 / 1, end states S-1 / S-2, the arcs of arcs()): the
    best score, accumulated in the DP's order (minus the arc's penalty, then plus the emission), or None when no path exists."""
    L = len(labels)
    S = 2 * L + 1
    T = len(em)
    pens = (0.0, float(penalty), float(repeat_penalty))
    lo, hi = _open(lo, hi, S, T)
    preds = arcs(labels, skip_from, repeat_from)
    succ = [[] for _ in range(S)]
    for s in range(S):
        for src, kind in preds[s]:
            if s == 0 and src != 0:
                continue
            succ[src].append((s, kind))
    col = [1 + s // 2 if s % 2 else 0 for s in range(S)]
    best = [None]

    def inside(t, s):
        return int(lo[s]) <= t < int(hi[s])

    def walk(t, s, score):
        if t == T - 1:
            if s in (S - 1, S - 2) and (best[0] is None or score > best[0]):
                best[0] = score
            return
        for nxt, kind in succ[s]:
            if not inside(t + 1, nxt):
                continue
            v = score - pens[kind] if kind else score
            walk(t + 1, nxt, v + float(em[t + 1][col[nxt]]))

    for s0 in (0, 1):
        if inside(0, s0):
            walk(0, s0, float(em[0][col[s0]]))
    return best[0]
