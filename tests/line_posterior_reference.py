"""tests/line_posterior_reference.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Forward-backward on the lattice of an unmarked lyric sheet (include/lyricalign.h la_alignment_posteriors_lines) as numpy float64 in the
log domain, over the ALL-PAIRS arc list: every plain arc, and a jump arc for every (source, target) pair the class rule allows that is
not a plain arc already.  Nothing of the kernel's hub -- the split of the plain arcs' weight, the sorted orders, the scans -- is restated
here.  The yardstick of tests/test_gpu_line_posteriors.py, itself pinned by tests/test_host_line_posteriors.py against exhaustive
enumeration of the lattice paths, against tests/posterior_reference.py (penalty +inf) and tests/repeat_posterior_reference.py (one line).

A path weighs exp(sum of its emissions) times: 1 per plain arc (k -> k, k -> k+1, k -> k+2 into an odd state whose neighbour label
differs), exp(-penalty) per jump arc; a start in state 0 or 1 weighs 1, in any other line-start state exp(-penalty); an end in S-1 or S-2
weighs 1, in any other jump source but state 0 exp(-penalty).
"""
from __future__ import annotations

import numpy as np

import line_order_reference as lor

NEG = -np.inf


def _lae(a, b):
    with np.errstate(invalid="ignore"):
        return np.logaddexp(a, b)


def _exp0(x):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.isnan(x) | np.isneginf(x), 0.0, np.exp(np.where(np.isnan(x), NEG, x)))


def _lse(m, axis):
    """log sum exp along an axis; an all -inf line gives -inf"""
    with np.errstate(invalid="ignore"):
        return np.logaddexp.reduce(m, axis=axis)


class Lattice:
    """The arcs of one sheet.  adv / skp [S]: the state has a plain advance / skip INTO it; src, tgt: the jump sources and targets in
    ascending order; jump [targets][sources]: that pair is a jump arc (allowed by the class rule and not a plain arc)."""

    def __init__(self, labels, line_start):
        labels = [int(v) for v in labels]
        self.labels, self.L = labels, len(labels)
        L, S = self.L, 2 * len(labels) + 1
        self.S = S
        self.starts = lor.line_starts_of(line_start, L)
        src, cls = lor.sources(labels, line_start)
        self.src = np.asarray(src, np.int64)
        self.tgt = np.asarray([2 * a + 1 for a in self.starts], np.int64)
        allowed = np.asarray([[c is None or c != labels[a] for c in cls] for a in self.starts], dtype=bool)
        self.adv = np.asarray([s >= 1 for s in range(S)], dtype=bool)
        self.skp = np.asarray([s % 2 == 1 and s >= 3 and labels[s // 2] != labels[s // 2 - 1] for s in range(S)], dtype=bool)
        plain = np.zeros_like(allowed)
        for i, k in enumerate(self.tgt):
            for j, s in enumerate(self.src):
                plain[i, j] = s == k - 1 or (s == k - 2 and self.skp[k])
        self.jump = allowed & ~plain
        self.col = np.asarray([1 + s // 2 if s % 2 else 0 for s in range(S)])
        self.start_cost = np.full(S, np.inf)          # penalty multiples charged at the start / the end; inf = not allowed
        self.start_cost[0] = self.start_cost[1] = 0.0
        for a in self.starts:
            if a != 0:
                self.start_cost[2 * a + 1] = 1.0
        self.end_cost = np.full(S, np.inf)
        for s in src:
            if s != 0:
                self.end_cost[s] = 1.0
        self.end_cost[S - 1] = self.end_cost[S - 2] = 0.0

    def charge(self, cost, penalty):
        """cost multiples -> log weights (0 * inf = 0: a free start stays free under a prohibitive penalty)"""
        with np.errstate(invalid="ignore"):
            return np.where(cost == 0.0, 0.0, np.where(np.isinf(cost), NEG, -cost * float(penalty)))


def _shift_r(row, by):
    return np.concatenate([np.full(by, NEG), row[:-by]]) if by < len(row) else np.full(len(row), NEG)


def _shift_l(row, by):
    return np.concatenate([row[by:], np.full(by, NEG)]) if by < len(row) else np.full(len(row), NEG)


def forward(em, lat, penalty):
    """-> e [T,S], alpha [T,S], inc [T,S] (arriving from another state), plain_in [T,S] (by a plain arc), log_z"""
    S, T = lat.S, np.asarray(em).shape[0]
    pen = float(penalty)
    e = np.asarray(em, np.float32)[:, lat.col].astype(np.float64)
    alpha = np.full((T, S), NEG)
    inc = np.full((T, S), NEG)
    plain_in = np.full((T, S), NEG)
    alpha[0] = e[0] + lat.charge(lat.start_cost, pen)
    for t in range(1, T):
        p = alpha[t - 1]
        i = _lae(np.where(lat.adv, _shift_r(p, 1), NEG), np.where(lat.skp, _shift_r(p, 2), NEG))
        plain_in[t] = i
        i = i.copy()
        with np.errstate(invalid="ignore"):
            vals = np.where(lat.jump, p[lat.src][None, :] - pen, NEG)
        i[lat.tgt] = _lae(i[lat.tgt], _lse(vals, 1))
        inc[t] = i
        alpha[t] = _lae(p, i) + e[t]
    log_z = float(_lse((alpha[T - 1] + lat.charge(lat.end_cost, pen))[None, :], 1)[0])
    return e, alpha, inc, plain_in, log_z


def log_z_only(em, labels, line_start, penalty=0.0):
    """The forward sweep alone (the wide lattices)."""
    return forward(em, Lattice(labels, line_start), penalty)[4]


def posteriors(em, labels, line_start, penalty=0.0):
    """em [T, >= L+1] compact float32 -> dict(gamma [T,S], entry [T,L], exit [T,L], visits [L], in_order [L], log_z).  Everything zero
    (log_z = -inf) when no path exists."""
    lat = Lattice(labels, line_start)
    L, S, T = lat.L, lat.S, np.asarray(em).shape[0]
    pen = float(penalty)
    e, alpha, inc, plain_in, log_z = forward(em, lat, pen)
    if np.isneginf(log_z):
        return dict(gamma=np.zeros((T, S)), entry=np.zeros((T, L)), exit=np.zeros((T, L)), visits=np.zeros(L), in_order=np.zeros(L),
                    log_z=log_z)
    beta = np.full((T, S), NEG)
    out = np.full((T, S), NEG)
    beta[T - 1] = e[T - 1] + lat.charge(lat.end_cost, pen)
    adv_from, skp_from = _shift_l(lat.adv.astype(float), 1) == 1.0, _shift_l(lat.skp.astype(float), 2) == 1.0
    for t in range(T - 2, -1, -1):
        q = beta[t + 1]
        o = _lae(np.where(adv_from, _shift_l(q, 1), NEG), np.where(skp_from, _shift_l(q, 2), NEG))
        with np.errstate(invalid="ignore"):
            vals = np.where(lat.jump, q[lat.tgt][:, None] - pen, NEG)
        o[lat.src] = _lae(o[lat.src], _lse(vals, 0))
        out[t] = o
        beta[t] = _lae(q, o) + e[t]
    odd = np.arange(1, S, 2)
    with np.errstate(invalid="ignore"):
        gamma = _exp0(alpha + beta - e - log_z)
        entry = _exp0(inc[:, odd] + beta[:, odd] - log_z)
        exit_ = _exp0(alpha[:, odd] + out[:, odd] - log_z)
        entry[0] = gamma[0, odd]
        exit_[T - 1] = gamma[T - 1, odd]
        in_order = np.zeros(L)
        for a in lat.starts:
            in_order[a] = _exp0(plain_in[1:, 2 * a + 1] + beta[1:, 2 * a + 1] - log_z).sum() + (gamma[0, 1] if a == 0 else 0.0)
    return dict(gamma=gamma, entry=entry, exit=exit_, visits=entry.sum(0), in_order=in_order, log_z=log_z)


def scores(ref, onset, offset, window):
    """occupancy, onset_prob, offset_prob of the reported (first-visit) segments, by the window logic of posterior_reference.scores."""
    import posterior_reference as pr
    return pr.scores(ref["gamma"], ref["entry"], ref["exit"], onset, offset, window)


def path_prob(ref, path):
    return np.asarray([ref["gamma"][t, s] for t, s in enumerate(path)], np.float64)


def brute(em, labels, line_start, penalty=0.0):
    """Every state sequence of a tiny lattice, weighed by the definition in the module text (linear domain) -> the dict of posteriors()."""
    lat = Lattice(labels, line_start)
    L, S, T = lat.L, lat.S, np.asarray(em).shape[0]
    q = float(np.exp(-float(penalty)))
    e = np.exp(np.asarray(em, np.float32)[:, lat.col].astype(np.float64))
    tgt_of = {int(k): i for i, k in enumerate(lat.tgt)}
    src_of = {int(s): j for j, s in enumerate(lat.src)}

    def arc(s, k):
        """-> (weight, arrives in print order) or None"""
        if k == s or k == s + 1 or (k == s + 2 and lat.skp[k]):
            return 1.0, k != s
        if k in tgt_of and s in src_of and lat.jump[tgt_of[k], src_of[s]]:
            return q, False
        return None

    Z = 0.0
    gamma = np.zeros((T, S)); entry = np.zeros((T, L)); exit_ = np.zeros((T, L)); in_order = np.zeros(L)

    def walk(path, w, ordered):
        nonlocal Z
        t, s = len(path) - 1, path[-1]
        if t == T - 1:
            c = lat.end_cost[s]
            if np.isinf(c):
                return
            w = w * (q if c else 1.0)
            if w == 0.0:
                return
            Z += w
            for u, k in enumerate(path):
                gamma[u, k] += w
                if k % 2 == 1:
                    if u == 0 or path[u - 1] != k:
                        entry[u, k // 2] += w
                    if u == T - 1 or path[u + 1] != k:
                        exit_[u, k // 2] += w
            for a in ordered:
                in_order[a] += w
            return
        for k in range(S):
            a = arc(s, k)
            if a is None or a[0] == 0.0:
                continue
            more = [k // 2] if (a[1] and k in tgt_of) else []
            walk(path + [k], w * a[0] * e[t + 1, k], ordered + more)

    for s0 in range(S):
        c = lat.start_cost[s0]
        if np.isinf(c):
            continue
        walk([s0], (q if c else 1.0) * e[0, s0], [0] if s0 == 1 else [])
    if Z == 0.0:
        return dict(gamma=np.zeros((T, S)), entry=np.zeros((T, L)), exit=np.zeros((T, L)), visits=np.zeros(L), in_order=np.zeros(L),
                    log_z=NEG)
    return dict(gamma=gamma / Z, entry=entry / Z, exit=exit_ / Z, visits=entry.sum(0) / Z, in_order=in_order / Z, log_z=float(np.log(Z)))
