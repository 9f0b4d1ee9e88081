"""tests/min_duration_reference.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The alignment DP on the plain lattice with a floor under every character's duration (include/lyricalign.h
la_viterbi_min_duration_batch) as numpy float64, one row at a time, vectorised over the labels of the row with every label's chain
padded to depth 8.  The yardstick of tests/test_gpu_min_duration.py (equality to the bit) and itself pinned by
tests/test_host_min_duration.py against exhaustive enumeration of the valid paths and, with every floor 1, against
tests/optional_spans_reference.py without spans.

States: 0 = leading silence, 2n+1 = label n, 2n+2 = the silence after label n; S = 2L+1.  floors[n] = D_n in 1 .. 8.  Label n has the
young values y_1 .. y_{D-1} (y_j: in its j-th frame; kept LEFT-aligned here, y_j in column j-1) and the mature value m (has lasted at
least D_n frames); only m is visible to the label's successors.
  row 0: sil_0 = em[0][0]; label 0: m = em[0][1] if D_0 == 1, else y_1 = em[0][1] and m = NEG; every other value NEG.
  row t (from row t-1; out_n = m_n, can_skip = n >= 1 and labels[n] != labels[n-1]):
      sil_0 stays; sil_{n+1} stays iff sil_{n+1} > out_n (strict), else it comes from out_n;
      D_n == 1: the plain rule on p0 = m_n, p1 = sil_n, p2 = out_{n-1}: skip iff can_skip and p2 >= p1 and p2 >= p0, else stay iff
          p0 > p1, else advance;
      D_n >= 2: entry = p2 if can_skip and p2 >= p1 else p1; y_1 = entry + em; y_j = y_{j-1} + em; m = (m > y_{D-1} ? m : y_{D-1}) + em.
  termination: 2L iff sil_L > m_{L-1} (strict), else the last label's mature value.
  backtrace: a mature cell that graduated at frame t puts the label on frames t-D+1 .. t and goes on from that first frame's entry.
  status: LA_OK iff the backtrace arrives at frame 0 in state 0 or in the first frame of label 0, else LA_EINFEASIBLE with every onset /
      offset -1 and an empty path (the score is still reported).
"""
from __future__ import annotations

import numpy as np

from optional_spans_reference import LA_EEMPTY, LA_EINFEASIBLE, LA_EINVAL, LA_OK, NEG  # noqa: F401  (re-exported for the tests)

DEPTH = 8          # the deepest floor; chains are padded to DEPTH - 1 young values


def lattice(em, labels, floors):
    """em [T][>= L+1] (float32 values) -> (sil [L+1], m [L]) of the last row, and per frame code [T][L] (the D == 1 cell's code or the
    D >= 2 entry's: 0 stay, 1 advance, 2 skip), grad [T][L] (the mature cell graduated) and sil_adv [T][L+1] (the silence came from the
    label before it)."""
    labels = np.asarray([int(v) for v in labels])
    L = len(labels)
    T = len(em)
    D = np.asarray([int(v) for v in floors])
    rows = np.asarray(em, dtype=np.float32)[:, : L + 1].astype(np.float64)
    can_skip = np.zeros(L, dtype=bool)
    can_skip[1:] = labels[1:] != labels[:-1]
    multi = D >= 2
    last = np.clip(D - 2, 0, DEPTH - 2)                     # the column of y_{D-1}
    idx = np.arange(L)
    sil = np.full(L + 1, NEG)
    m = np.full(L, NEG)
    y = np.full((L, DEPTH - 1), NEG)
    sil[0] = rows[0, 0]
    if D[0] == 1:
        m[0] = rows[0, 1]
    else:
        y[0, 0] = rows[0, 1]
    code = np.zeros((T, L), dtype=np.int8)
    grad = np.zeros((T, L), dtype=bool)
    sil_adv = np.zeros((T, L + 1), dtype=bool)
    for t in range(1, T):
        e = rows[t, 1:]
        p0, p1 = m, sil[:L]
        p2 = np.concatenate([[NEG], m[:-1]])
        # D == 1: the plain rule
        skip = can_skip & (p2 >= p1) & (p2 >= p0)
        stay = p0 > p1
        best1 = np.where(skip, p2, np.where(stay, p0, p1))
        code1 = np.where(skip, 2, np.where(stay, 0, 1))
        # D >= 2: the entry and the chain
        via = can_skip & (p2 >= p1)
        entry = np.where(via, p2, p1)
        ylast = y[idx, last]
        stay_m = p0 > ylast
        best_m = np.where(stay_m, p0, ylast)
        y_new = np.empty_like(y)
        y_new[:, 1:] = y[:, :-1] + e[:, None]
        y_new[:, 0] = entry + e
        m_new = np.where(multi, best_m, best1) + e
        # silences
        sil_new = np.empty_like(sil)
        sil_new[0] = sil[0] + rows[t, 0]
        stay_s = sil[1:] > m
        sil_new[1:] = np.where(stay_s, sil[1:], m) + rows[t, 0]
        code[t] = np.where(multi, np.where(via, 2, 1), code1)
        grad[t] = multi & ~stay_m
        sil_adv[t, 1:] = ~stay_s
        sil, m, y = sil_new, m_new, y_new
    return sil, m, code, grad, sil_adv


def viterbi(em, labels, floors):
    """-> (onset [L], offset [L], score, status, path).  LA_EINVAL (score 0.0) for a floor outside 1 .. 8."""
    L = len(labels)
    if L == 0:
        return [], [], 0.0, LA_EEMPTY, []
    T = len(em)
    if T <= 0 or len(floors) < L or any(int(v) < 1 or int(v) > DEPTH for v in floors[:L]):
        return [-1] * L, [-1] * L, 0.0, LA_EINVAL, []
    floors = [int(v) for v in floors[:L]]
    sil, m, code, grad, sil_adv = lattice(em, labels, floors)
    kk = 2 * L if sil[L] > m[L - 1] else 2 * L - 1
    score = float(sil[L] if kk == 2 * L else m[L - 1])
    onset, offset, path = [-1] * L, [-1] * L, [-1] * T
    bad = ([-1] * L, [-1] * L, score, LA_EINFEASIBLE, [])
    j = T - 1
    while True:
        n = kk >> 1
        if kk & 1 and floors[n] >= 2:
            t = j
            while t > 0 and not grad[t, n]:
                t -= 1
            f = t - floors[n] + 1
            if t == 0 or f < 0:
                return bad
            onset[n], offset[n] = f, j + 1
            path[f: j + 1] = [kk] * (j + 1 - f)
            if f == 0:
                if kk != 1:
                    return bad
                break
            kk -= int(code[f, n])
            j = f - 1
        else:
            path[j] = kk
            if kk & 1 and offset[n] < 0:
                offset[n] = j + 1
            if j == 0:
                if kk > 1:
                    return bad
                if kk & 1:
                    onset[n] = 0
                break
            c = int(code[j, n]) if kk & 1 else (0 if kk == 0 else int(sil_adv[j, n]))
            if kk & 1 and c != 0:
                onset[n] = j
            kk -= c
            j -= 1
    return onset, offset, score, LA_OK, path


def plain(em, labels):
    """The plain lattice: every floor 1."""
    return viterbi(em, labels, [1] * len(labels))


def enumerate_best(em, labels, floors):
    """Exhaustive walk over every VALID path of a tiny lattice: it tracks the run length of the current label and refuses to leave a
    label, or to end in it, before its floor.  -> the best score, accumulated in the DP's order, or None where no valid path exists."""
    labels = [int(v) for v in labels]
    floors = [int(v) for v in floors]
    L = len(labels)
    S = 2 * L + 1
    T = len(em)
    col = [1 + s // 2 if s % 2 else 0 for s in range(S)]
    best = [None]

    def walk(t, s, run, score):
        if t == T - 1:
            if s == S - 1 or (s == S - 2 and run >= floors[s // 2]):
                if best[0] is None or score > best[0]:
                    best[0] = score
            return
        for k in (s, s + 1, s + 2):
            if k >= S or (k == s + 2 and not (k % 2 == 1 and labels[k // 2] != labels[k // 2 - 1])):
                continue
            if k != s and s % 2 == 1 and run < floors[s // 2]:
                continue
            walk(t + 1, k, run + 1 if k == s else 1, score + float(em[t + 1][col[k]]))

    for s0 in (0, 1):
        walk(0, s0, 1, float(em[0][col[s0]]))
    return best[0]


# ------------------------------------------------------------------------------------------------ planted clips (shared by the tests)
FLOOR_POOL = (1, 2, 3, 4, 5, 6, 7, 8, 1, 2, 3, 4, 2, 3, 1, 2)       # every value 1 .. 8, mean 3.4 frames


def weak_tail(seed, L, T, seg=4, floors=None, max_floor=8, gap_every=7, gap=2, vocab=1000, equal_pair=True, pair_at=None):
    """One planted clip with WEAK TAILS: seg frames per label, `gap` frames of silence in front of every gap_every-th label, silence up
    to T.  The sung cell is -0.1, every other cell -8 (plus continuous noise: ties have measure zero).  Every second label that does
    not follow a silence is clear only in its first frame (its own cell -0.1, the previous label's -0.5 as its vowel rings on);
    afterwards its own cell sits near -3 and the previous label's near -2.5 -- the plain lattice keeps the previous label through that
    tail and gives this one a single frame.  floors: given, or drawn from FLOOR_POOL (values above max_floor left out) until the tight
    path fits into T.  equal_pair: labels q - 1 and q (q = pair_at, or L // 2) are made equal, with floors >= 2 where they were drawn.
    -> dict(lab, em [T, L+1] float32, floors, T, onset, offset (the planted truth), weak)."""
    rs = np.random.RandomState(seed)
    lab = [int(v) for v in rs.randint(1, vocab + 1, size=L)]
    for n in range(1, L):
        if lab[n] == lab[n - 1]:
            lab[n] = lab[n] % vocab + 1
    q = L // 2 if pair_at is None else int(pair_at)
    if equal_pair and L >= 2:
        lab[q] = lab[q - 1]
        if q + 1 < L and lab[q + 1] == lab[q]:
            lab[q + 1] = lab[q] % vocab + 1
    pairs = sum(1 for n in range(1, L) if lab[n] == lab[n - 1])
    if floors is None:
        pool = [v for v in FLOOR_POOL if v <= max_floor]
        while True:
            floors = [int(v) for v in rs.choice(pool, size=L)]
            if equal_pair and L >= 2:
                floors[q - 1], floors[q] = max(2, floors[q - 1]), max(2, floors[q])
            if sum(floors) + pairs <= T:
                break
    floors = [int(v) for v in floors]
    truth, onset, offset, weak = [], [], [], []
    for n in range(L):
        after_silence = n == 0 or n % gap_every == 0
        if n and after_silence:
            truth += [0] * gap
        onset.append(len(truth))
        truth += [1 + n] * seg
        offset.append(len(truth))
        weak.append(n % 2 == 1 and not after_silence)
    assert len(truth) <= T, (len(truth), T)
    truth += [0] * (T - len(truth))
    em = -8.0 + rs.normal(0.0, 0.3, size=(T, L + 1))
    em[np.arange(T), truth] = -0.1 + rs.normal(0.0, 0.01, size=T)
    for n in range(L):
        if weak[n]:
            f0 = onset[n]
            em[f0, n] = -0.5 + rs.normal(0.0, 0.02)                      # (column n = label n-1)
            for f in range(f0 + 1, offset[n]):
                em[f, 1 + n] = -3.0 + rs.normal(0.0, 0.05)
                em[f, n] = -2.5 + rs.normal(0.0, 0.05)
    return dict(lab=lab, em=np.ascontiguousarray(em.astype(np.float32)), floors=floors, T=T, onset=onset, offset=offset, weak=weak)


def short_of_floor(onset, offset, floors):
    """How many labels hold fewer frames than their floor."""
    return sum(1 for a, b, d in zip(onset, offset, floors) if b - a < d)


def boundary_error(onset, offset, clip):
    """Mean |frames| between the reported and the planted onsets and offsets."""
    return float(np.mean([abs(a - x) + abs(b - z) for a, b, x, z in zip(onset, offset, clip["onset"], clip["offset"])]))
