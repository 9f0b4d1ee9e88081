"""CPU yardstick of the alignment posteriors (helper, not collected as a test): float64 numpy forward-backward on the
lattice of utils/alignment.py (sum-product where the DP is max-product), the DP itself, and a brute-force enumerator of
all paths for lattices small enough to enumerate.  Definitions: include/lyricalign.h, la_alignment_posteriors.
"""
import itertools

import numpy as np

NEG = -np.inf


def lattice(labels):
    """-> S, skip[k] (k-2 -> k allowed), col[k] (compact emission column of state k)."""
    L = len(labels)
    S = 2 * L + 1
    skip = np.zeros(S, bool)
    for k in range(3, S, 2):
        skip[k] = labels[k // 2] != labels[k // 2 - 1]
    col = np.zeros(S, np.int64)
    for k in range(1, S, 2):
        col[k] = 1 + k // 2
    return S, skip, col


def _lse3(a, b, c):
    m = np.maximum(a, np.maximum(b, c))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = m + np.log(np.exp(a - m) + np.exp(b - m) + np.exp(c - m))
    return np.where(np.isneginf(m), NEG, r)


def fwd_bwd(em, labels):
    """em [T, >= L+1] compact float32 -> alpha, beta [T,S] float64 (both include e_t(k)), e [T,S], log_z, skip."""
    T = em.shape[0]
    S, skip, col = lattice(labels)
    e = np.asarray(em)[:, col].astype(np.float64)
    alpha = np.full((T, S), NEG)
    alpha[0, 0] = e[0, 0]
    alpha[0, 1] = e[0, 1]
    for t in range(1, T):
        p0 = alpha[t - 1]
        p1 = np.concatenate([[NEG], p0[:-1]])
        p2 = np.where(skip, np.concatenate([[NEG, NEG], p0[:-2]]), NEG)
        alpha[t] = _lse3(p0, p1, p2) + e[t]
    beta = np.full((T, S), NEG)
    beta[T - 1, S - 1] = e[T - 1, S - 1]
    beta[T - 1, S - 2] = e[T - 1, S - 2]
    skip_from = np.concatenate([skip[2:], [False, False]])   # k -> k+2 allowed
    for t in range(T - 2, -1, -1):
        n0 = beta[t + 1]
        n1 = np.concatenate([n0[1:], [NEG]])
        n2 = np.where(skip_from, np.concatenate([n0[2:], [NEG, NEG]]), NEG)
        beta[t] = _lse3(n0, n1, n2) + e[t]
    log_z = np.logaddexp(alpha[T - 1, S - 1], alpha[T - 1, S - 2])
    return alpha, beta, e, log_z, skip


def _exp0(v):
    with np.errstate(invalid="ignore"):
        return np.nan_to_num(np.exp(v), nan=0.0)


def posteriors(em, labels):
    """-> gamma [T,S], entry [T,L], exit [T,L], log_z.  entry[t][n] = P(first frame of label n is t), exit: last frame.
    All zero (log_z = -inf) when no path exists."""
    alpha, beta, e, log_z, skip = fwd_bwd(em, labels)
    T, S = alpha.shape
    L = len(labels)
    if np.isneginf(log_z):
        return np.zeros((T, S)), np.zeros((T, L)), np.zeros((T, L)), log_z
    gamma = _exp0(alpha + beta - e - log_z)
    odd = np.arange(1, S, 2)
    entry = np.zeros((T, L))
    exit_ = np.zeros((T, L))
    entry[0] = gamma[0, odd]
    exit_[T - 1] = gamma[T - 1, odd]
    if T > 1:
        with np.errstate(invalid="ignore"):
            inc = np.logaddexp(alpha[:-1, odd - 1], np.where(skip[odd], alpha[:-1, np.maximum(odd - 2, 0)], NEG))
            entry[1:] = _exp0(inc + beta[1:, odd] - log_z)
            nxt = np.minimum(odd + 2, S - 1)
            skip_out = np.where(odd + 2 < S, skip[nxt], False)
            out = np.logaddexp(beta[1:, odd + 1], np.where(skip_out, beta[1:, nxt], NEG))
            exit_[:-1] = _exp0(alpha[:-1, odd] + out - log_z)
    return gamma, entry, exit_, log_z


def viterbi(em, labels):
    """The DP of utils/alignment.py (comparison order and tie rules of run_viterbi_core) -> onset, offset (frames), score."""
    T = em.shape[0]
    S, skip, col = lattice(labels)
    e = np.asarray(em)[:, col].astype(np.float64)
    dp = np.full((T, S), -1e7)
    bt = np.zeros((T, S), int)
    dp[0, 0] = e[0, 0]
    dp[0, 1] = e[0, 1]
    for j in range(1, T):
        for k in range(S):
            p0 = dp[j - 1, k]
            p1 = dp[j - 1, k - 1] if k >= 1 else None
            p2 = dp[j - 1, k - 2] if k >= 2 else None
            if k == 0:
                bt[j, k] = 0; best = p0
            elif k % 2 == 1 and k >= 3 and skip[k] and p2 >= p1 and p2 >= p0:
                bt[j, k] = k - 2; best = p2
            elif p0 > p1:
                bt[j, k] = k; best = p0
            else:
                bt[j, k] = k - 1; best = p1
            dp[j, k] = best + e[j, k]
    kk = S - 1 if dp[-1, -1] > dp[-1, -2] else S - 2
    score = dp[-1, kk]
    path = [kk]
    for j in range(T - 1, 0, -1):
        kk = bt[j, kk]
        path.append(kk)
    path.reverse()
    L = len(labels)
    on = [path.index(2 * n + 1) if (2 * n + 1) in path else -1 for n in range(L)]
    off = [T - path[::-1].index(2 * n + 1) if (2 * n + 1) in path else -1 for n in range(L)]
    return on, off, score


def scores(gamma, entry, exit_, onset, offset, window):
    """The three per-label outputs of la_alignment_posteriors from the full posteriors and the DP's frames."""
    T = gamma.shape[0]
    L = entry.shape[1]
    occ, onp, offp = np.zeros(L), np.zeros(L), np.zeros(L)
    for n in range(L):
        a, b = int(onset[n]), int(offset[n])
        if a < 0 or b <= a:
            continue
        occ[n] = gamma[a:b, 2 * n + 1].mean()
        onp[n] = entry[max(a - window, 0): min(a + window, T - 1) + 1, n].sum()
        last = b - 1
        offp[n] = exit_[max(last - window, 0): min(last + window, T - 1) + 1, n].sum()
    return occ, onp, offp


def brute(em, labels):
    """All paths of a small lattice -> gamma [T,S], log_z."""
    T = em.shape[0]
    S, skip, col = lattice(labels)
    e = np.asarray(em)[:, col].astype(np.float64)
    Z = 0.0
    occ = np.zeros((T, S))
    for path in itertools.product(range(S), repeat=T):
        if path[0] > 1 or path[-1] < S - 2:
            continue
        ok = True
        for t in range(1, T):
            d = path[t] - path[t - 1]
            if d == 0 or d == 1 or (d == 2 and skip[path[t]]):
                continue
            ok = False
            break
        if not ok:
            continue
        w = np.exp(sum(e[t, path[t]] for t in range(T)))
        Z += w
        for t in range(T):
            occ[t, path[t]] += w
    return occ / Z, np.log(Z)


def fix_repeats(em, labels):
    """Compact-layout contract: equal neighbouring labels read one class column."""
    for n in range(1, len(labels)):
        if labels[n] == labels[n - 1]:
            em[:, 1 + n] = em[:, n]
    return em


def make_inputs(T, L, scale, seed, flat=False):
    """Peaked emissions around a random ground-truth segmentation (so that the posterior is not flat), one repeated
    neighbour pair.  flat: no segment bonus (2L segment edges do not fit into T frames)."""
    rs = np.random.RandomState(seed)
    labels = list(int(v) for v in rs.randint(1, 400, size=L))
    labels[L // 2] = labels[L // 2 - 1]
    em = (-rs.rand(T, L + 1) * scale - 1.0).astype(np.float32)
    if not flat:
        bounds = np.sort(rs.choice(np.arange(1, T), size=2 * L, replace=False))
        for n in range(L):
            em[bounds[2 * n]:bounds[2 * n + 1], 1 + n] += scale * 0.8
    return fix_repeats(em, labels), labels
