"""CPU yardstick of the alignment posteriors on the lattice with optional label spans (helper, not collected as a test): float64 numpy
forward-backward over the arcs of tests/optional_spans_reference.py::arcs (sum-product where la_viterbi_spans_batch is max-product; a jump
arc weighs exp(-penalty)), the per-label scores with the window logic of tests/posterior_reference.py, and a brute-force enumerator of all
paths for lattices small enough to enumerate.  Definitions: include/lyricalign.h, la_alignment_posteriors_spans.
"""
import numpy as np

import optional_spans_reference as osr
import posterior_reference as pr

NEG = -np.inf


def arc_arrays(labels, skip_from):
    """-> src, dst, jump: one entry per arc of the lattice (self loops included), in osr.arcs' order."""
    preds = osr.arcs(labels, skip_from)
    src, dst, jump = [], [], []
    for s, plist in enumerate(preds):
        for a, j in plist:
            src.append(a)
            dst.append(s)
            jump.append(j)
    return np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(jump, bool)


def _emissions(em, L):
    S = 2 * L + 1
    col = np.zeros(S, np.int64)
    col[1::2] = 1 + np.arange(L)
    return np.asarray(em)[:, col].astype(np.float64)


def _lse_at(S, idx, vals):
    acc = np.full(S, NEG)
    with np.errstate(invalid="ignore"):
        np.logaddexp.at(acc, idx, vals)
    return acc


def posteriors(em, labels, skip_from, penalty=0.0):
    """em [T, >= L+1] compact float32 -> gamma [T,S], entry [T,L], exit [T,L], present [L], span_skip [L+1] (indexed by the span's end
    position, 0 where no span ends), log_z.  alpha and beta both include e_t(k).  All zero (log_z = -inf) when no path exists."""
    labels = [int(v) for v in labels]
    L = len(labels)
    S = 2 * L + 1
    T = np.asarray(em).shape[0]
    penalty = float(penalty)
    e = _emissions(em, L)
    src, dst, jump = arc_arrays(labels, skip_from)
    cost = np.where(jump, penalty, 0.0)
    other = src != dst
    alpha = np.full((T, S), NEG)
    alpha[0, 0] = e[0, 0]
    alpha[0, 1] = e[0, 1]
    inc = np.full((T, S), NEG)              # log weight of arriving in k at frame t from another state
    for t in range(1, T):
        vals = alpha[t - 1, src] - cost
        alpha[t] = _lse_at(S, dst, vals) + e[t]
        inc[t] = _lse_at(S, dst[other], vals[other])
    beta = np.full((T, S), NEG)
    beta[T - 1, S - 1] = e[T - 1, S - 1]
    beta[T - 1, S - 2] = e[T - 1, S - 2]
    out = np.full((T, S), NEG)              # log weight of leaving k after frame t for another state
    for t in range(T - 2, -1, -1):
        vals = beta[t + 1, dst] - cost
        beta[t] = _lse_at(S, src, vals) + e[t]
        out[t] = _lse_at(S, src[other], vals[other])
    log_z = np.logaddexp(alpha[T - 1, S - 1], alpha[T - 1, S - 2])
    if np.isneginf(log_z):
        return np.zeros((T, S)), np.zeros((T, L)), np.zeros((T, L)), np.zeros(L), np.zeros(L + 1), log_z
    odd = np.arange(1, S, 2)
    with np.errstate(invalid="ignore"):
        gamma = pr._exp0(alpha + beta - e - log_z)
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


def scores(gamma, entry, exit_, onset, offset, window):
    """The three windowed per-label outputs (labels with onset -1: 0), by the window logic of posterior_reference.scores."""
    return pr.scores(gamma, entry, exit_, onset, offset, window)


def spans_of(skip_from):
    """skip_from [L+1] -> [(a, n)] in ascending n; out-of-range entries are none."""
    return [(int(a), n) for n, a in enumerate(skip_from) if 0 <= int(a) < n]


def coverage(present, span_skip, skip_from):
    """present[n] + the mass of every span that covers n: 1 for every label (a monotone path leaves n out only by one such jump)."""
    cov = np.array(present, dtype=np.float64)
    for a, n in spans_of(skip_from):
        cov[a:n] += span_skip[n]
    return cov


def brute(em, labels, skip_from, penalty=0.0):
    """All paths of a small lattice -> gamma [T,S], log_z, present [L], span_skip [L+1]."""
    labels = [int(v) for v in labels]
    L = len(labels)
    S = 2 * L + 1
    T = np.asarray(em).shape[0]
    penalty = float(penalty)
    e = _emissions(em, L)
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
            walk(path + [nxt], score - (penalty if j else 0.0) + e[t, nxt], jumps + [nxt // 2] if j else jumps)

    for s0 in (0, 1):
        walk([s0], e[0, s0], [])
    return occ / z[0], np.log(z[0]), present / z[0], skip / z[0]


def make_inputs(T, line_lengths, absent, scale, seed, lean):
    """posterior_reference.make_inputs for a lyric sheet of lines: label columns lowered by `lean`; ground-truth segments (bonus
    0.8 * scale + lean) only for the characters of lines not in `absent`; one repeated neighbour pair; every line an optional span.
    -> em [T, L+1] float32, labels [L], skip_from [L+1]."""
    rs = np.random.RandomState(seed)
    lengths = [int(v) for v in line_lengths]
    L = sum(lengths)
    labels = list(int(v) for v in rs.randint(1, 400, size=L))
    labels[L // 2] = labels[L // 2 - 1]
    em = (-rs.rand(T, L + 1) * scale - 1.0).astype(np.float32)
    em[:, 1:] -= np.float32(lean)
    starts = np.cumsum([0] + lengths)
    sung = [n for i in range(len(lengths)) if i not in absent for n in range(starts[i], starts[i + 1])]
    bounds = np.sort(rs.choice(np.arange(1, T), size=2 * len(sung), replace=False))
    for i, n in enumerate(sung):
        em[bounds[2 * i]:bounds[2 * i + 1], 1 + n] += np.float32(scale * 0.8 + lean)
    skip_from = [-1] * (L + 1)
    for i in range(len(lengths)):
        skip_from[int(starts[i + 1])] = int(starts[i])
    return pr.fix_repeats(em, labels), labels, skip_from


# The inputs of tests/test_gpu_span_posteriors.py's generator cases; tests/test_host_span_posteriors.py asserts that their span_skip
# values cover certain (> 0.99), impossible (< 0.01) and undecided ([0.05, 0.95]) -- otherwise the device test would be vacuous.
GENERATOR_CASES = [                   # (T, line_lengths, absent, scale, seed, lean)
    (150, [3] * 5, {2}, 3.0, 3, 0.3),
    (150, [3] * 5, {2}, 3.0, 3, 6.0),
    (40, [2, 2], {1}, 3.0, 7, 6.0),
    (40, [2, 2], {0}, 3.0, 7, 0.3),
]
PENALTIES = (0.0, 1.0)
