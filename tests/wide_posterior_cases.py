"""Case builders of tests/test_gpu_wide_posteriors.py (helper, not collected as a test):
the lattices of la_alignment_posteriors_lattice beyond 511 labels with their float64 yardstick -- window_posterior_reference.posteriors
for gamma, entry, exit, present, span skip and log_z, span_posterior_reference.scores for the three windowed per-label outputs, on the
onset / offset of windows_reference.viterbi_windows(..., rows=True).  Everything is computed once per shape on the host and shared:
lattice_case hands out the cached arrays read-only and its lists as copies.
"""
import functools

import numpy as np

import window_posterior_reference as wpr
import windows_reference as wr
from test_gpu_windows import _emissions, _labels

# (T, L): the first strip shape (S = 1025 leaves thread 512 with one valid state) at four frame counts, so that every prefetch depth in
# use (4, 2, 1) meets a ragged last block; the R = 2 to 4 edge; the R = 4 to 8 edge
SHAPES = [(560, 512), (561, 512), (562, 512), (563, 512), (1100, 1023), (1100, 1024), (2200, 2047), (2200, 2048)]


def labels_of(seed, L):
    """_labels plus one equal-neighbour pair at labels 63 / 64.  A thread's first state k0 = tid * R is even (R is 2, 4 or 8), so a label's
    state 2n+1 is never the first state of a thread; label 64's state 129 is the first LABEL state (r = 1) of its thread at every R, and
    of a wave at R = 2: its k-2 neighbour, the state of label 63 that the equal-neighbour rule closes, belongs to the previous thread and
    arrives through the exchanged row."""
    lab = _labels(seed, L)
    if L > 64:
        lab[64] = lab[63]
    return lab


def span_set(L):
    """skip_from [L+1] for L >= 512 holding: a span starting at label 0 (no J-1); a one-label span (the source lies in the reader's own
    strip); a nested pair; two spans sharing a start (source state 80 has four targets: out-degree above 2); a span of 310 labels (source
    and target lie in different waves at every R: a wave holds at most 256 labels); spans every 30 labels; a span ending at position L;
    the long arc lists of long_arc_lists."""
    assert L >= 512
    skip = [-1] * (L + 1)
    skip[3] = 0
    skip[8] = 7
    skip[30], skip[25] = 10, 15
    skip[50], skip[56] = 40, 40
    skip[400] = 90
    for n in range(450, L - 10, 30):
        skip[n] = n - 4
    skip[L] = L - 5
    return long_arc_lists(skip)


def long_arc_lists(skip):
    """Adds to skip_from [L+1], L >= 140, the spans that give one thread of the strip kernel more than the four arc words it keeps in
    registers, so that the part of the backward fold that reads the list from the workspace runs.  Three spans share the start 101: the
    source state 202 has six targets, state 201 (label 100, the J-1 source) up to six more, and 101 is odd, so both belong to one thread
    at R = 4 and 8 and to neighbouring threads at R = 2.  Two spans start at the adjacent labels 105 and 106: their source states 209 ..
    212 belong to one thread at R = 8.  The lists of the threads of that wave have different lengths (arc_list_lengths)."""
    assert len(skip) > 140 and all(skip[n] < 0 for n in (110, 115, 120, 130, 135))
    skip[110] = skip[115] = skip[120] = 101
    skip[130], skip[135] = 105, 106
    return skip


def arc_list_lengths(skip, lab, R):
    """Jump arcs by source thread for R states per thread -> int array [1024]: what posterior_strip_kernel's thread folds per backward
    step.  A span (a, m) leaves state 2a for 2m and (m < L) 2m+1, and state 2a-1 (a >= 1) for 2m and, where the labels differ, 2m+1."""
    L = len(lab)
    n = np.zeros(1024, np.int64)
    for m in range(1, L + 1):
        a = skip[m]
        if not 0 <= a < m:
            continue
        n[2 * a // R] += 1 + (m < L)
        if a >= 1:
            n[(2 * a - 1) // R] += 1 + (m < L and lab[m] != lab[a - 1])
    return n


def strip_states_per_thread(max_labels):
    return 2 if max_labels <= 1023 else 4 if max_labels <= 2047 else 8


def assert_long_arc_lists(skip, lab, R):
    """The lattice gives a thread more arc words than the four held in registers, and the lists of that thread's wave differ in length
    (shorter lists are padded to the wave's maximum).  -> the lengths above four in that wave."""
    n = arc_list_lengths(skip, lab, R)
    wave = n[int(n.argmax()) // 64 * 64:][:64]
    assert wave.max() > 4 and 0 < sorted(set(wave))[-2] < wave.max(), (R, wave.tolist())
    return sorted(int(x) for x in wave if x > 4)


def narrowed_windows(em, lab, skip, pen):
    """Open windows except that two states of the open-window DP's path (the one it holds at frame T // 2 and its last one) are narrowed
    to their segment of that path, as window_posterior_reference.edge_cases does."""
    T, L = em.shape[0], len(lab)
    lo, hi = wr.open_windows(L, T)
    base = wr.viterbi_windows(em, lab, lo, hi, skip, pen, rows=True)
    assert base[3] == wr.LA_OK
    path = list(base[4])
    for s in {path[T // 2], path[-1]}:
        lo[s], hi[s] = path.index(s), T - path[::-1].index(s)
    return lo, hi


def yardstick(em, lab, skip, pen, lo=None, hi=None):
    """-> dict(on, off, score, status, ref): the DP's frames and wpr.posteriors on the same lattice (lo None: every window open)."""
    T, L = em.shape[0], len(lab)
    if lo is None:
        lo, hi = wr.open_windows(L, T)
    on, off, score, status, _ = wr.viterbi_windows(em, lab, lo, hi, skip, pen, rows=True)
    return dict(on=on, off=off, score=score, status=status, ref=wpr.posteriors(em, lab, lo, hi, skip, pen))


LATTICES = ["open windows", "spans, penalty 0", "spans, penalty 0.5", "spans and windows"]


def _frozen(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, tuple):
        for y in x:
            _frozen(y)
    return x


def lattice_case(T, L, v):
    """Lattice v of one shape: 0 no spans with every window open (given), 1 / 2 the span set at penalties 0 / 0.5 without windows, 3 the span
    set at 0.5 with the narrowed windows.  -> dict(name, skip, pen, lab, em, lo, hi, on, off, score, status, ref); lo / hi None: no windows
    are given to the entry.  Computed once: a fresh dict per call, its lists copies, its arrays the cached ones, read-only."""
    return {k: list(x) if isinstance(x, list) else _frozen(x) for k, x in _lattice_case(T, L, v).items()}


@functools.lru_cache(maxsize=None)
def _lattice_case(T, L, v):
    lab = labels_of(7 * T + L, L)
    sheet = span_set(L)
    name = LATTICES[v]
    skip, pen, win = [(None, 0.0, "open"), (sheet, 0.0, None), (sheet, 0.5, None), (sheet, 0.5, "narrow")][v]
    em = _emissions(500 + v + T, T, lab, 1.0 * (v % 2))
    lo = hi = None
    if win == "open":
        lo, hi = wr.open_windows(L, T)
    elif win == "narrow":
        lo, hi = narrowed_windows(em, lab, skip, pen)
    y = yardstick(em, lab, skip, pen, lo, hi)
    assert y["status"] == wr.LA_OK and np.isfinite(y["ref"][5]), (T, L, name)
    return dict(name=name, skip=skip, pen=pen, lab=lab, em=em, lo=lo, hi=hi, **y)


def every_line_optional(L, line=10):
    skip = [-1] * (L + 1)
    for n in range(line, L + 1, line):
        skip[n] = n - line
    if skip[L] < 0:
        skip[L] = L - L % line
    return skip


def forward_log_z(em, lab, skip, pen):
    """A forward-only float64 sweep of the span lattice (no windows) -> log_z.  Written apart from the yardstick: at 4095 labels the full
    yardstick takes 14 s and 2.7 GB, this takes a few seconds."""
    lab = np.asarray(lab)
    T, L = em.shape[0], len(lab)
    S = 2 * L + 1
    col = np.zeros(S, np.int64)
    col[1::2] = 1 + np.arange(L)
    e = np.asarray(em)[:, col].astype(np.float64)
    can_skip = np.zeros(S, bool)
    can_skip[3::2] = lab[1:] != lab[:-1]
    tgt, src = [], []                                   # jump arcs: target state, source state
    for n in range(1, L + 1):
        a = skip[n]
        if not 0 <= a < n:
            continue
        for k in ((2 * n, 2 * n + 1) if n < L else (2 * n,)):
            tgt.append(k); src.append(2 * a)
            if a >= 1 and (k % 2 == 0 or lab[n] != lab[a - 1]):
                tgt.append(k); src.append(2 * a - 1)
    tgt, src = np.asarray(tgt, np.int64), np.asarray(src, np.int64)
    alpha = np.full(S, -np.inf)
    alpha[:2] = e[0, :2]
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            a1 = np.concatenate([[-np.inf], alpha[:-1]])
            a2 = np.where(can_skip, np.concatenate([[-np.inf, -np.inf], alpha[:-2]]), -np.inf)
            new = np.logaddexp(np.logaddexp(alpha, a1), a2)
            if len(tgt):
                np.logaddexp.at(new, tgt, alpha[src] - pen)
            alpha = new + e[t]
    return float(np.logaddexp(alpha[S - 1], alpha[S - 2]))
