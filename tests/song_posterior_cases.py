"""Case builders of tests/test_host_song_posteriors.py and tests/test_gpu_song_posteriors.py (helper, not collected as a test): what
la_alignment_posteriors_song needs beyond the helpers of the repeat lattice (tests/test_gpu_repeat_spans.py, repeat_posterior_reference)
and of the wide lattices (wide_posterior_cases) -- the documented workspace size, a forward-only float64 sweep of the repeat lattice for
the largest shape, sheets whose arc lists mix skip and repeat words, and the arc-list lengths with the repeat arcs."""
import numpy as np

import repeat_spans_reference as rr
import wide_posterior_cases as wpc


def workspace_bytes(batch, max_frames, max_labels):
    """include/lyricalign.h la_alignment_posteriors_song: up to 511 labels the alpha rows of the lane-per-state form; beyond, alpha rows,
    6 float64 sums per label and 3 arc words per state."""
    S = 2 * max_labels + 1
    if max_labels <= 511:
        nw = 1
        while nw * 64 < S:
            nw *= 2
        return batch * max_frames * nw * 64 * 8
    NS = 1024 * wpc.strip_states_per_thread(max_labels)
    return batch * max_frames * NS * 8 + batch * (NS // 2) * 6 * 8 + batch * 3 * NS * 4


def forward_log_z(em, lab, skip=None, pen=0.0, rf=None, rpen=0.0):
    """A forward-only float64 sweep of the lattice with optional and repeatable spans (no windows) -> log_z, built on
    repeat_spans_reference.arcs: at 4095 labels the full yardstick is too large to keep, this takes a few seconds."""
    L = len(lab)
    S = 2 * L + 1
    T = em.shape[0]
    col = np.zeros(S, np.int64)
    col[1::2] = 1 + np.arange(L)
    src, dst, cost = [], [], []
    for s, preds in enumerate(rr.arcs(list(lab), skip, rf)):
        for k, kind in preds:
            src.append(k); dst.append(s); cost.append((0.0, float(pen), float(rpen))[kind])
    src, dst, cost = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(cost, np.float64)
    alpha = np.full(S, -np.inf)
    alpha[:2] = np.asarray(em[0], np.float64)[col[:2]]
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            new = np.full(S, -np.inf)
            np.logaddexp.at(new, dst, alpha[src] - cost)
            alpha = new + np.asarray(em[t], np.float64)[col]
    return float(np.logaddexp(alpha[S - 1], alpha[S - 2]))


# the repeat spans added to wide_posterior_cases.span_set: two that END at position 101, where three optional spans start (state 202 is
# the J of six skip arcs and the K of both; state 201 their J-1 / K-1), and a pair at the adjacent ends 105 and 106, where two more start
MIXED_REPEATS = ((95, 101), (97, 101), (103, 105), (104, 106))


def mixed_sheet(L):
    """-> skip_from [L+1] (wide_posterior_cases.span_set), repeat_from [L] and the sung sequence that takes every repeat span once."""
    skip = wpc.span_set(L)
    rf = [-1] * L
    for a, e in MIXED_REPEATS:
        rf[a] = e
    parts = [list(range(0, 101)), list(range(95, 101)), list(range(97, 101)) + list(range(101, 105)), list(range(103, 105)) + [105],
             [104, 105] + list(range(106, L))]
    return skip, rf, [n for part in parts for n in part]


def breaths_of(lab, sung):
    """Where the planting needs a frame of silence in front of sung[i]: before every return (the arc through the silence exists whatever
    the labels) and between equal labels (the lattice has no arc from a label to an equal neighbour)."""
    return [i for i in range(1, len(sung)) if sung[i] <= sung[i - 1] or lab[sung[i]] == lab[sung[i - 1]]]


def repeat_arc_words(rf, lab, R):
    """Repeat arcs by source -> {source state: [target states, ascending]}: the span (a, e) leaves state 2e, and 2e-1 where the labels of
    a and e-1 differ, for 2a+1."""
    out = {}
    L = len(lab)
    for a in range(L):
        e = rf[a]
        if not a < e <= L:
            continue
        out.setdefault(2 * e, []).append(2 * a + 1)
        if lab[a] != lab[e - 1]:
            out.setdefault(2 * e - 1, []).append(2 * a + 1)
    return out


def arc_list_lengths(skip, rf, lab, R):
    """wide_posterior_cases.arc_list_lengths plus the repeat arcs: what the REP face's thread folds per backward step."""
    n = wpc.arc_list_lengths(skip, lab, R)
    for s, targets in repeat_arc_words(rf, lab, R).items():
        n[s // R] += len(targets)
    return n


def assert_mixed_arc_lists(skip, rf, lab, R):
    """One thread folds more than four words, among them skip words followed by at least two repeat words of ONE state, and other lists
    of its wave are shorter.  -> that thread's list length."""
    n = arc_list_lengths(skip, rf, lab, R)
    reps = repeat_arc_words(rf, lab, R)
    skips = wpc.arc_list_lengths(skip, lab, R)
    s = 202                                            # J of the spans starting at 101, K of the repeat spans ending there
    assert len(reps.get(s, [])) >= 2 and skip[110] == skip[115] == skip[120] == 101
    tid = s // R
    assert n[tid] > 4 and skips[tid] >= 6 and n[tid] >= skips[tid] + 2, (R, int(n[tid]), int(skips[tid]))
    wave = n[tid // 64 * 64:][:64]
    assert wave.max() == n[tid] and (wave < wave.max()).any() and (wave[wave < wave.max()] > 0).any(), (R, wave.tolist())
    return int(n[tid])


def truth_of(em):
    """The planted lattice column per frame of a hard planted clip (0: silence, 1 + n: label n)."""
    return [int(np.flatnonzero(row == np.float32(-0.25))[0]) for row in em]
