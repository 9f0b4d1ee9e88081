"""Yardstick for the pronunciation alternatives (include/lyricalign.h la_emissions_merge_readings / la_reading_scores): the float64 fold
of a position's readings into the merged class, the sequential segment sums, the reading rule and the set-equality ids, restated in
plain numpy / Python.  The DP and the posteriors have their own restatements (repeat_spans_reference and friends): they run on the
folded matrix unchanged."""
import math

import numpy as np

READING_SET_ID = 1 << 24


def fold64(x):
    """x: the float32 emissions of one position's A >= 1 readings at one frame -> the merged emission BEFORE rounding, a float64:
    m + log(sum_a exp(x_a - m)) with m the float maximum, summed in ascending a; -inf if m is -inf.  One reading: the value itself."""
    x = [np.float32(v) for v in x]
    if len(x) == 1:
        return np.float64(x[0])
    m = -np.inf
    for v in x:
        if v > m:
            m = v
    if m == -np.inf:
        return np.float64(-np.inf)
    s = 0.0
    for v in x:
        s += math.exp(float(v) - float(m))
    return np.float64(float(m) + math.log(s))


def fold_rows64(em_x, alt_start):
    """em_x [T, 1 + columns] float32, alt_start [L + 1] -> float64 [T, L + 1]: column 0 and single readings are the input's values, the
    others fold64 of their group, vectorised over the frames in the same order of operations (maximum, then ascending-a sum)."""
    em_x = np.asarray(em_x, dtype=np.float32)
    T, L = em_x.shape[0], len(alt_start) - 1
    out = np.empty((T, L + 1), dtype=np.float64)
    out[:, 0] = em_x[:, 0]
    for n in range(L):
        g = em_x[:, 1 + alt_start[n]: 1 + alt_start[n + 1]].astype(np.float64)
        if g.shape[1] == 1:
            out[:, 1 + n] = g[:, 0]
            continue
        m = g.max(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.zeros(T)
            for a in range(g.shape[1]):
                s = s + np.exp(g[:, a] - m)
            out[:, 1 + n] = np.where(np.isneginf(m), -np.inf, m + np.log(s))
    return out


def fold_rows(em_x, alt_start):
    """fold_rows64 rounded once to float32: what the kernel writes, up to one float32 step where the float64 value lies within a few
    float64 ulps of a rounding boundary."""
    return fold_rows64(em_x, alt_start).astype(np.float32)


def segment_scores(em_x, alt_start, onset, offset):
    """-> col_score [columns] float64: per expanded column the sum of em_x[t, 1 + j] over t ascending in [onset, offset) of its position,
    accumulated sequentially (np.cumsum adds in order; np.sum would add pairwise); 0 for a skipped position (onset -1)."""
    em_x = np.asarray(em_x, dtype=np.float32)
    out = np.zeros(int(alt_start[-1]), dtype=np.float64)
    for n in range(len(alt_start) - 1):
        if onset[n] < 0 or offset[n] <= onset[n]:
            continue
        for j in range(alt_start[n], alt_start[n + 1]):
            out[j] = np.cumsum(em_x[onset[n]: offset[n], 1 + j].astype(np.float64))[-1]
    return out


def pick_readings(col_score, alt_start, onset):
    """-> reading [L]: the smallest index with the largest score among the position's readings, -1 for a skipped position."""
    out = []
    for n in range(len(alt_start) - 1):
        if onset[n] < 0:
            out.append(-1)
            continue
        best = 0
        for a in range(1, alt_start[n + 1] - alt_start[n]):
            if col_score[alt_start[n] + a] > col_score[alt_start[n] + best]:
                best = a
        out.append(best)
    return out


def lattice_ids(sets):
    """sets[n] = the class ids of position n, the sheet's own first -> the ids the lattice compares: the class itself for a single
    reading, READING_SET_ID + k for the k-th distinct multi-reading set (compared as sets, numbered by first appearance)."""
    known, out = {}, []
    for r in sets:
        if len(r) == 1:
            out.append(int(r[0]))
        else:
            out.append(READING_SET_ID + known.setdefault(frozenset(int(c) for c in r), len(known)))
    return out
