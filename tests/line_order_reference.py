"""tests/line_order_reference.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The alignment DP on the lattice of an unmarked lyric sheet (include/lyricalign.h la_viterbi_lines_batch) as numpy float64, in its
ALL-PAIRS form: every jump target looks at every allowed jump source of the previous row -- nothing of the kernel's hub is restated
here.  The yardstick of tests/test_gpu_line_order.py (equality to the bit) and itself pinned by tests/test_host_line_order.py against
exhaustive enumeration of the lattice paths, against tests/optional_spans_reference.py (penalty +inf) and against
tests/repeat_spans_reference.py (one line).

States: 0 = leading silence, 2n+1 = label n, 2n+2 = the silence after label n; S = 2L+1.  line_start[n] != 0: label n begins a line
(entry 0 must).  The line ends E are the starts other than 0, and L.
  jump sources: state 0 and, for every e in E, 2e-1 and 2e; class labels[s >> 1] for an odd source, "none" for a silence.
  jump targets: 2a+1 for every line start a, from any source of row t-1 whose class differs from labels[a]; the largest raw value wins,
      the smallest state among equals; taken only if that value minus the penalty is STRICTLY greater than the neighbour rule's winner.
  free start: row 0 is the plain lattice's, and every line start a != 0 gets em[0][1+a] - penalty.
  free end: S-1 against S-2 (strict >) first; then the best source other than 0, S-1, S-2 replaces it only if its value minus the
      penalty is strictly greater.
Backpointer codes: 0 stay, 1 advance, 2 skip, 3 jump.
"""
from __future__ import annotations

import numpy as np

from optional_spans_reference import LA_EEMPTY, LA_EINFEASIBLE, LA_EINVAL, LA_OK, NEG  # noqa: F401  (re-exported for the tests)

NINF = float("-inf")


def line_starts_of(line_start, L):
    """The flag row -> the label indices that begin a line."""
    return [n for n in range(L) if int(line_start[n]) != 0]


def sources(labels, line_start):
    """-> the jump sources in ascending state order, and the class of each (None for a silence)."""
    L = len(labels)
    starts = line_starts_of(line_start, L)
    ends = starts[1:] + [L]
    src = sorted({0} | {2 * e - 1 for e in ends} | {2 * e for e in ends})
    return src, [labels[s >> 1] if s & 1 else None for s in src]


def lattice(em, labels, line_start, penalty):
    """em [T][>= L+1] (float32 values) -> dp [T][S] float64, bt [T][S] (predecessor state), code [T][S]; one row at a time, every target
    against every source."""
    labels = [int(v) for v in labels]
    L = len(labels)
    S = 2 * L + 1
    T = len(em)
    penalty = float(penalty)
    starts = line_starts_of(line_start, L)
    src, src_cls = sources(labels, line_start)
    src = np.asarray(src)
    tgt = np.asarray([2 * a + 1 for a in starts])
    allowed = np.asarray([[c is None or c != labels[a] for c in src_cls] for a in starts], dtype=bool)          # [targets][sources]
    may_skip = np.asarray([s % 2 == 1 and s >= 3 and labels[s // 2] != labels[s // 2 - 1] for s in range(S)], dtype=bool)
    col = np.asarray([1 + s // 2 if s % 2 else 0 for s in range(S)])
    rows = np.asarray(em, dtype=np.float32)[:, : L + 1].astype(np.float64)
    states = np.arange(S)
    dp = np.empty((T, S), dtype=np.float64)
    bt = np.zeros((T, S), dtype=np.int64)
    codes = np.zeros((T, S), dtype=np.int64)
    prev = np.full((S,), NEG)
    prev[0], prev[1] = rows[0, 0], rows[0, 1]
    for a in starts:
        if a != 0:
            prev[2 * a + 1] = rows[0, 1 + a] - penalty
    dp[0] = prev
    for t in range(1, T):
        p0 = prev
        p1 = np.concatenate([[NEG], prev[:-1]])
        p2 = np.concatenate([[NEG, NEG], prev[:-2]])
        skip = may_skip & (p2 >= p1) & (p2 >= p0)
        stay = p0 > p1
        best = np.where(skip, p2, np.where(stay, p0, p1))
        code = np.where(skip, 2, np.where(stay, 0, 1))
        back = states - code
        best[0], back[0], code[0] = p0[0], 0, 0
        # all pairs: the first maximum along the ascending sources is the smallest state among equals
        vals = np.where(allowed, prev[src][None, :], NINF)
        pick = np.argmax(vals, axis=1)
        v = vals[np.arange(len(tgt)), pick] - penalty          # (a row without an allowed source: -inf, never strictly greater)
        take = v > best[tgt]
        best[tgt] = np.where(take, v, best[tgt])
        back[tgt] = np.where(take, src[pick], back[tgt])
        code[tgt] = np.where(take, 3, code[tgt])
        cur = best + rows[t, col]
        dp[t], bt[t], codes[t] = cur, back, code
        prev = cur
    return dp, bt, codes


class Result(tuple):
    """(onset, offset, score, status, path) -- and what the tests' preconditions ask about the path."""
    n_jumps = 0            # jump arcs taken between two frames
    free_start = False     # the path begins at a line start other than label 0
    free_end = False       # the path ends in a source other than S-1 / S-2


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


def viterbi(em, labels, line_start, penalty=0.0):
    """-> Result (onset [L], offset [L], score, status, path): a label's FIRST visit in time, -1 / -1 for a label never visited, LA_OK
    even then.  LA_EINVAL (score 0.0, an empty path) where line_start[0] is zero."""
    L = len(labels)
    if L == 0:
        return Result(([], [], 0.0, LA_EEMPTY, []))
    T = len(em)
    if T <= 0 or int(line_start[0]) == 0:
        return Result(([-1] * L, [-1] * L, 0.0, LA_EINVAL, []))
    S = 2 * L + 1
    penalty = float(penalty)
    dp, bt, codes = lattice(em, labels, line_start, penalty)
    fin = dp[T - 1]
    kk = S - 1 if fin[S - 1] > fin[S - 2] else S - 2
    score = float(fin[kk])
    free_end = False
    cand = [s for s in sources(labels, line_start)[0] if s not in (0, S - 1, S - 2)]
    if cand:
        s = cand[int(np.argmax(fin[cand]))]
        if float(fin[s]) - penalty > score:
            kk, score, free_end = s, float(fin[s]) - penalty, True
    path = [kk]
    n_jumps = 0
    for t in range(T - 1, 0, -1):
        n_jumps += int(codes[t][kk]) == 3
        kk = int(bt[t][kk])
        path.append(kk)
    path.reverse()
    onset, offset = [-1] * L, [-1] * L
    for n, first, end in segments(path):
        if onset[n] < 0:
            onset[n], offset[n] = first, end
    r = Result((onset, offset, score, LA_OK, path))
    r.n_jumps, r.free_start, r.free_end = n_jumps, path[0] > 1, free_end
    return r


def line_order(path, line_start, L):
    """The line index of every occurrence in time order: a new occurrence begins where a visit does not continue the line's last one."""
    starts = line_starts_of(line_start, L)
    line_of = [sum(1 for a in starts if a <= n) - 1 for n in range(L)]
    order, last = [], None
    for n, _, _ in segments(path):
        if last is None or line_of[last] != line_of[n] or n <= last:
            order.append(line_of[n])
        last = n
    return order


def enumerate_best(em, labels, line_start, penalty):
    """Exhaustive search over every path of the lattice (tiny ones only): the best score, accumulated in the DP's order."""
    labels = [int(v) for v in labels]
    L = len(labels)
    S = 2 * L + 1
    T = len(em)
    penalty = float(penalty)
    starts = line_starts_of(line_start, L)
    src, src_cls = sources(labels, line_start)
    cls_of = dict(zip(src, src_cls))
    col = [1 + s // 2 if s % 2 else 0 for s in range(S)]

    def arcs(s):
        """-> [(next state, is a jump)]; a target reachable both ways takes the better, i.e. the free, arc"""
        out = {}
        for k in range(S):
            if s in cls_of and k % 2 == 1 and k // 2 in starts and (cls_of[s] is None or cls_of[s] != labels[k // 2]):
                out[k] = True
            if k == s or k == s + 1 or (k == s + 2 and k % 2 == 1 and labels[k // 2] != labels[k // 2 - 1]):
                out[k] = False
        return out.items()

    best = [None]

    def walk(t, s, score):
        if t == T - 1:
            if s in (S - 1, S - 2):
                pass
            elif s in cls_of and s != 0:
                score = score - penalty
            else:
                return
            if best[0] is None or score > best[0]:
                best[0] = score
            return
        for nxt, jump in arcs(s):
            v = score - penalty if jump else score
            walk(t + 1, nxt, v + float(em[t + 1][col[nxt]]))

    for s0 in range(S):
        if s0 <= 1:
            walk(0, s0, float(em[0][col[s0]]))
        elif s0 % 2 == 1 and s0 // 2 in starts:
            walk(0, s0, float(em[0][col[s0]]) - penalty)
    return best[0]


# ------------------------------------------------------------------------------------------------ planted performances (shared by the tests)
def flags_of_lengths(lengths):
    """Line lengths -> the line_start flag row."""
    row = []
    for n in lengths:
        row += [1] + [0] * (int(n) - 1)
    return row


def planted(seed, T, lengths, sung_lines, seg=3, gap=2, vocab=40, labels=None):
    """One clip of a sheet with the given line lengths, sung as the lines `sung_lines` in that order: seg frames per label, gap frames of
    silence after every line, silence up to T.  The sung cell is -0.1, every other cell -8, both plus continuous noise (ties have measure
    zero).  -> dict(lab, em [T, L+1] float32, ls, T, sung)."""
    rs = np.random.RandomState(seed)
    L = int(sum(lengths))
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(int)
    lab = [int(v) for v in (rs.randint(1, vocab + 1, size=L) if labels is None else labels)]
    truth = []
    for m in sung_lines:
        for n in range(starts[m], starts[m + 1]):
            truth += [1 + n] * seg
        truth += [0] * gap
    assert len(truth) <= T, (len(truth), T)
    truth += [0] * (T - len(truth))
    em = -8.0 + rs.normal(0.0, 0.3, size=(T, L + 1))
    em[np.arange(T), truth] = -0.1 + rs.normal(0.0, 0.01, size=T)
    return dict(lab=lab, em=np.ascontiguousarray(em.astype(np.float32)), ls=flags_of_lengths(lengths), T=T, sung=list(sung_lines))
