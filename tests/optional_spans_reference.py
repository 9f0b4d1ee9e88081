"""tests/optional_spans_reference.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The alignment DP on the lattice with optional label spans (include/lyricalign.h la_viterbi_spans_batch) as plain Python
float64: recurrence, backtrace, marking of skipped labels, status.  The yardstick of tests/test_gpu_optional_spans.py
(equality to the bit) and itself pinned by tests/test_host_optional_spans.py against oracle/viterbi_python.py (no spans)
and against exhaustive enumeration of lattice paths (with spans).

States: 0 = leading silence, 2n+1 = label n, 2n+2 = the silence after label n; S = 2L+1.  skip_from[n] = a with
0 <= a < n makes labels a..n-1 optional: states 2n and 2n+1 (n < L) may also be entered from J = 2a and, when a >= 1 (and,
for 2n+1, labels[n] != labels[a-1]), from J-1.  Both arcs cost `penalty` and win only if strictly greater, J first.
"""
from __future__ import annotations

NEG = -10000000.0
LA_OK, LA_EINVAL, LA_EINFEASIBLE, LA_EEMPTY = 0, 1, 2, 3


def jump_sources(labels, skip_from):
    """-> J[s] (2a, or -1 for none), jm1[s] (arc from J-1 allowed) for the S = 2L+1 states.  Out-of-range entries are none."""
    L = len(labels)
    S = 2 * L + 1
    J, jm1 = [-1] * S, [False] * S
    for s in range(2, S):
        n = s // 2
        a = int(skip_from[n])
        if 0 <= a < n:
            J[s] = 2 * a
            jm1[s] = a >= 1 and (s % 2 == 0 or labels[n] != labels[a - 1])
    return J, jm1


def arcs(labels, skip_from):
    """-> preds[s] = list of (source state, is_jump) in the lattice (enumeration and tests)."""
    L = len(labels)
    S = 2 * L + 1
    J, jm1 = jump_sources(labels, skip_from)
    preds = []
    for s in range(S):
        p = [(s, False)]
        if s >= 1:
            p.append((s - 1, False))
        if s % 2 == 1 and s >= 3 and labels[s // 2] != labels[s // 2 - 1]:
            p.append((s - 2, False))
        if J[s] >= 0:
            p.append((J[s], True))
            if jm1[s]:
                p.append((J[s] - 1, True))
        preds.append(p)
    return preds


def lattice(em, labels, skip_from, penalty=0.0):
    """em [T][>= L+1] (float32 values), -> dp [T][S] (Python floats = float64), bt [T][S] (predecessor state),
    jumped [T][S] (the predecessor was reached over a span's arc)."""
    L = len(labels)
    S = 2 * L + 1
    T = len(em)
    penalty = float(penalty)
    J, jm1 = jump_sources(labels, skip_from)
    may_skip = [s % 2 == 1 and s >= 3 and labels[s // 2] != labels[s // 2 - 1] for s in range(S)]
    col = [1 + s // 2 if s % 2 else 0 for s in range(S)]
    rows = [[float(v) for v in em[t][: L + 1]] for t in range(T)]
    prev = [NEG] * S
    prev[0] = rows[0][0]
    prev[1] = rows[0][1]
    dp, bt, jumped = [prev], [[0] * S], [[False] * S]
    for t in range(1, T):
        e = rows[t]
        cur, src_row, jump_row = [0.0] * S, [0] * S, [False] * S
        cur[0] = prev[0] + e[0]
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
            cur[s] = best + e[col[s]]
            src_row[s] = src
            jump_row[s] = jump
        dp.append(cur)
        bt.append(src_row)
        jumped.append(jump_row)
        prev = cur
    return dp, bt, jumped


def viterbi_spans(em, labels, skip_from, penalty=0.0):
    """-> (onset [L], offset [L], score, status, path).  Labels inside a taken jump: -1 / -1 with LA_OK."""
    L = len(labels)
    if L == 0:
        return [], [], 0.0, LA_EEMPTY, []
    T = len(em)
    if T <= 0:
        return [-1] * L, [-1] * L, 0.0, LA_EINVAL, []
    S = 2 * L + 1
    labels = [int(v) for v in labels]
    dp, bt, jumped = lattice(em, labels, skip_from, penalty)
    kk = S - 1 if dp[T - 1][S - 1] > dp[T - 1][S - 2] else S - 2
    score = dp[T - 1][kk]
    path = [kk]
    skipped = [False] * L
    for t in range(T - 1, 0, -1):
        src = bt[t][kk]
        if jumped[t][kk]:                         # labels a .. n-1 of the span that ends at position n = kk // 2
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


def enumerate_best(em, labels, skip_from, penalty=0.0):
    """Exhaustive search over every lattice path (start states 0 / 1, end states S-1 / S-2, arcs of arcs()): the best score,
    accumulated in the DP's order (minus penalty on a jump, then plus the emission), or None when no path exists."""
    L = len(labels)
    S = 2 * L + 1
    T = len(em)
    penalty = float(penalty)
    preds = arcs(labels, skip_from)
    succ = [[] for _ in range(S)]
    for s in range(S):
        for src, jump in preds[s]:
            if s == 0 and src != 0:
                continue
            succ[src].append((s, jump))
    col = [1 + s // 2 if s % 2 else 0 for s in range(S)]
    best = [None]

    def walk(t, s, score):
        if t == T - 1:
            if s in (S - 1, S - 2) and (best[0] is None or score > best[0]):
                best[0] = score
            return
        for nxt, jump in succ[s]:
            v = score - penalty if jump else score
            walk(t + 1, nxt, v + float(em[t + 1][col[nxt]]))

    for s0 in (0, 1):
        walk(0, s0, float(em[0][col[s0]]))
    return best[0]
