"""tests/repeat_posterior_reference.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

CPU yardstick of the alignment posteriors on the lattice with REPEATABLE label spans (include/lyricalign.h
la_alignment_posteriors_repeats): a float64 numpy forward-backward over the arcs of tests/repeat_spans_reference.py::arcs (plain arcs,
an optional span's jumps at skip_penalty, a repeat span's returns at repeat_penalty -- imported, not restated) with the window gate of
tests/window_posterior_reference.py, and a brute-force enumerator of the paths for lattices small enough to enumerate.

The repeat arcs point left, but the sweep is frame-synchronous: (frame, state) is still a DAG.  A path may visit a label more than once,
so entry / exit / visits / repeat_count / span_skip are EXPECTED COUNTS (a visit = a maximal run of frames in one odd state):
  entry[t][n]      a visit of label n begins at frame t (a repeat arc into 2n+1 is an entry, and an exit of its source)
  visits[n]        sum_t entry[t][n]
  repeat_count[a]  the path takes a repeat arc into 2a+1: sum over t >= 1 and the sources of exp(alpha[t-1][src] - repeat_penalty
                   + beta[t][2a+1] - log_z)
  span_skip[n]     the path takes a jump of the optional span that ends at position n
and for every label n   visits[n] + sum of span_skip[e'] over optional spans a' <= n < e'  =  1 + sum of repeat_count[a] over repeat
spans a <= n < e   (identity_sides).
"""
import numpy as np

import posterior_reference as pr
import repeat_spans_reference as rr
import window_posterior_reference as wpr
import windows_reference as wr

NEG = -np.inf


def _arc_arrays(labels, skip_from, repeat_from):
    """-> src, dst, kind (0 plain, 1 skip jump, 2 repeat) of every arc of rr.arcs, self loops included."""
    src, dst, kind = [], [], []
    for s, plist in enumerate(rr.arcs(labels, skip_from, repeat_from)):
        for a, k in plist:
            src.append(a); dst.append(s); kind.append(k)
    return np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(kind, np.int64)


def _lse_at(S, idx, vals):
    acc = np.full(S, NEG)
    with np.errstate(invalid="ignore"):
        np.logaddexp.at(acc, idx, vals)
    return acc


def _lae(a, b):
    with np.errstate(invalid="ignore"):
        return np.logaddexp(a, b)


def posteriors(em, labels, skip_from=None, penalty=0.0, repeat_from=None, repeat_penalty=0.0, lo=None, hi=None):
    """em [T, >= L+1] compact float32; lo / hi [>= 2L+1] or None (open) -> dict(gamma [T,S], entry [T,L], exit [T,L], visits [L],
    span_skip [L+1], repeat_count [L], log_z).  Everything zero (log_z = -inf) when no path exists."""
    labels = [int(v) for v in labels]
    L = len(labels)
    S = 2 * L + 1
    T = np.asarray(em).shape[0]
    if lo is None:
        lo, hi = wr.open_windows(L, T)
    e = np.asarray(em)[:, [1 + s // 2 if s % 2 else 0 for s in range(S)]].astype(np.float64)
    eg = np.where(wpr.inside(T, S, lo, hi), e, NEG)
    src, dst, kind = _arc_arrays(labels, skip_from, repeat_from)
    cost = np.where(kind == 1, float(penalty), np.where(kind == 2, float(repeat_penalty), 0.0))
    # the plain arcs as two shifted rows (the lists of a wide lattice are long); the few jump / repeat arcs one by one
    adv = np.zeros(S, bool); skp = np.zeros(S, bool)
    plain = kind == 0
    adv[dst[plain & (src == dst - 1)]] = True
    skp[dst[plain & (src == dst - 2)]] = True
    assert (plain == (plain & ((src == dst) | (src == dst - 1) | (src == dst - 2)))).all()
    far = ~plain
    fs, fd, fc, fk = src[far], dst[far], cost[far], kind[far]

    def shift_r(row, by):                      # row[s - by]
        return np.concatenate([np.full(by, NEG), row[:-by]]) if by < len(row) else np.full(len(row), NEG)

    def shift_l(row, by):                      # row[s + by]
        return np.concatenate([row[by:], np.full(by, NEG)]) if by < len(row) else np.full(len(row), NEG)

    alpha = np.full((T, S), NEG)
    alpha[0, 0] = eg[0, 0]
    alpha[0, 1] = eg[0, 1]
    inc = np.full((T, S), NEG)                 # log weight of arriving in k at frame t from another state
    for t in range(1, T):
        p = alpha[t - 1]
        i = _lae(np.where(adv, shift_r(p, 1), NEG), np.where(skp, shift_r(p, 2), NEG))
        if len(fs):
            i = _lae(i, _lse_at(S, fd, p[fs] - fc))
        inc[t] = i
        alpha[t] = _lae(p, i) + eg[t]
    beta = np.full((T, S), NEG)
    beta[T - 1, S - 1] = eg[T - 1, S - 1]
    beta[T - 1, S - 2] = eg[T - 1, S - 2]
    out = np.full((T, S), NEG)                 # log weight of leaving k after frame t for another state
    adv_from, skp_from = shift_l(adv.astype(float), 1) == 1.0, shift_l(skp.astype(float), 2) == 1.0
    for t in range(T - 2, -1, -1):
        q = beta[t + 1]
        o = _lae(np.where(adv_from, shift_l(q, 1), NEG), np.where(skp_from, shift_l(q, 2), NEG))
        if len(fs):
            o = _lae(o, _lse_at(S, fs, q[fd] - fc))
        out[t] = o
        beta[t] = _lae(q, o) + eg[t]
    log_z = np.logaddexp(alpha[T - 1, S - 1], alpha[T - 1, S - 2])
    zero = dict(gamma=np.zeros((T, S)), entry=np.zeros((T, L)), exit=np.zeros((T, L)), visits=np.zeros(L), span_skip=np.zeros(L + 1),
                repeat_count=np.zeros(L), log_z=log_z)
    if np.isneginf(log_z):
        return zero
    odd = np.arange(1, S, 2)
    with np.errstate(invalid="ignore"):
        gamma = pr._exp0(alpha + beta - e - log_z)      # the unmasked emission; alpha = beta = -inf outside the window: 0
        entry = pr._exp0(inc[:, odd] + beta[:, odd] - log_z)
        exit_ = pr._exp0(alpha[:, odd] + out[:, odd] - log_z)
        entry[0] = gamma[0, odd]
        exit_[T - 1] = gamma[T - 1, odd]
        span_skip, repeat_count = np.zeros(L + 1), np.zeros(L)
        if T > 1 and len(fs):
            mass = pr._exp0(alpha[:-1][:, fs] - fc + beta[1:][:, fd] - log_z).sum(0)
            np.add.at(span_skip, fd[fk == 1] // 2, mass[fk == 1])
            np.add.at(repeat_count, fd[fk == 2] // 2, mass[fk == 2])
    return dict(gamma=gamma, entry=entry, exit=exit_, visits=entry.sum(0), span_skip=span_skip, repeat_count=repeat_count, log_z=log_z)


def scores(ref, onset, offset, window):
    """occupancy, onset_prob, offset_prob of the reported (first-visit) segments, by the window logic of posterior_reference.scores."""
    return pr.scores(ref["gamma"], ref["entry"], ref["exit"], onset, offset, window)


def path_prob(ref, path):
    """gamma at the reported path -> [len(path)]."""
    return np.asarray([ref["gamma"][t, s] for t, s in enumerate(path)], np.float64)


def repeat_spans_of(repeat_from, L):
    return [] if repeat_from is None else [(a, int(repeat_from[a])) for a in range(L) if a < int(repeat_from[a]) <= L]


def skip_spans_of(skip_from):
    return [] if skip_from is None else [(int(a), n) for n, a in enumerate(skip_from) if 0 <= int(a) < n]


def identity_sides(visits, span_skip, repeat_count, skip_from, repeat_from):
    """-> (visits[n] + the skip mass of every optional span over n, 1 + the return mass of every repeat span over n), each [L]."""
    L = len(visits)
    left = np.array(visits, np.float64)
    right = np.ones(L)
    for a, n in skip_spans_of(skip_from):
        left[a:n] += span_skip[n]
    for a, e in repeat_spans_of(repeat_from, L):
        right[a:e] += repeat_count[a]
    return left, right


def brute(em, labels, skip_from=None, penalty=0.0, repeat_from=None, repeat_penalty=0.0, lo=None, hi=None):
    """All paths of a small lattice inside the windows -> the dict of posteriors(), counted path by path; None when no path exists."""
    labels = [int(v) for v in labels]
    L = len(labels)
    S = 2 * L + 1
    T = np.asarray(em).shape[0]
    if lo is None:
        lo, hi = wr.open_windows(L, T)
    e = np.asarray(em)[:, [1 + s // 2 if s % 2 else 0 for s in range(S)]].astype(np.float64)
    ok = wpr.inside(T, S, lo, hi)
    pens = (0.0, float(penalty), float(repeat_penalty))
    succ = [[] for _ in range(S)]
    for s, plist in enumerate(rr.arcs(labels, skip_from, repeat_from)):
        for a, k in plist:
            succ[a].append((s, k))
    gamma, entry, exit_ = np.zeros((T, S)), np.zeros((T, L)), np.zeros((T, L))
    span_skip, repeat_count = np.zeros(L + 1), np.zeros(L)
    z = [0.0]

    def walk(path, kinds, score):
        t = len(path)
        if t == T:
            if path[-1] >= S - 2:
                w = np.exp(score)
                z[0] += w
                for tt, s in enumerate(path):
                    gamma[tt, s] += w
                    if s % 2:
                        if tt == 0 or path[tt - 1] != s:
                            entry[tt, s // 2] += w
                        if tt == T - 1 or path[tt + 1] != s:
                            exit_[tt, s // 2] += w
                    if kinds[tt] == 1:
                        span_skip[s // 2] += w
                    elif kinds[tt] == 2:
                        repeat_count[s // 2] += w
            return
        for nxt, k in succ[path[-1]]:
            if ok[t, nxt]:
                walk(path + [nxt], kinds + [k], score - pens[k] + e[t, nxt])

    for s0 in (0, 1):
        if s0 < S and ok[0, s0]:
            walk([s0], [0], e[0, s0])
    if z[0] == 0.0:
        return None
    Z = z[0]
    return dict(gamma=gamma / Z, entry=entry / Z, exit=exit_ / Z, visits=entry.sum(0) / Z, span_skip=span_skip / Z,
                repeat_count=repeat_count / Z, log_z=np.log(Z))
