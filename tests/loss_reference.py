"""Float64 restatement of la_multitask_loss (include/lyricalign.h: word CE, silence BCE and CTC on the align logits, and their gradient on
the logits), its float32 yardstick, and the case table that tests/test_host_loss_kernels.py and tests/test_gpu_loss_kernels.py share.
Importable without a GPU; plain torch and numpy.

losses_and_grad is written from the header's contract, not from the kernels: the CE and BCE terms are a few torch ops, the CTC term a
hand-written alpha / beta sweep over the 2L+1 states (one numpy row per frame).  tests/test_host_loss_kernels.py pins it to float64
torch (log_softmax + F.ctc_loss, F.cross_entropy, F.binary_cross_entropy_with_logits under autograd) wherever torch defines the case.
It also defines what torch does not:
  * a clip without labels: nll 0, no gradient, and the batch mean is still divided by B;
  * a clip without a path (fewer frames than labels plus adjacent repeats, or a label whose class lies outside 0..V-1): nll +inf,
    losses[2] +inf, the clip's CTC gradient rows exactly zero, its batch mates untouched;
  * a frame label outside 1..V-1 (other than -100): the frame does not count for the word CE and has no CE gradient; for the silence BCE
    it is a frame with a label (target 0);
  * no frame with a label: losses[0] NaN, the word-CE gradient zero, the BCE gradient intact.
A term that was not requested (use_ce / use_ctc) is NaN here; the entry's value for it is not part of the contract.

e32 is the yardstick of the GPU test's rule err <= 8 x E32: the same quantity with every row normaliser taken by torch in FLOAT32 on the
CPU (torch.log_softmax for the CTC term, F.cross_entropy and F.binary_cross_entropy_with_logits under float32 autograd for the frame
terms) and cast to double, the lattice running in float64 on those values -- the error no float32 row pass can avoid.  losses and dlogits
are then rounded to float32, the format in which the entry returns them; nll stays double.  Nothing in it depends on the code under test.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from row_kernel_reference import rel_err  # noqa: F401  (the losses' error measure; re-exported)

MODES = {"ce": (1, 0, 1.0), "ctc": (0, 1, 1.0), "both": (1, 1, 0.125)}      # use_ce, use_ctc, scale


def grad_err(a: torch.Tensor, ref: torch.Tensor) -> float:
    """max |a - ref| relative to the tensor's largest |ref| (ref float64, not all zero)."""
    a, ref = a.detach().double(), ref.detach().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float((a - ref).abs().max() / ref.abs().max())


# ---- the CTC lattice of one clip ----------------------------------------------------------------------------------------------------

def _lse(*rows):
    """log sum exp over the given rows, elementwise; -inf where all are -inf."""
    x = np.stack(rows)
    m = x.max(0)
    safe = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return safe + np.log(np.exp(x - safe).sum(0))


def _shift_down(a, k):
    """row[s] <- a[s - k], -inf for s < k"""
    return np.concatenate([np.full(k, -np.inf), a[:-k]])


def _shift_up(a, k):
    """row[s] <- a[s + k], -inf past the end"""
    return np.concatenate([a[k:], np.full(k, -np.inf)])


def ctc_clip(logp: np.ndarray, labels, V: int):
    """logp [T, V] float64: log-softmax over columns 0..V-1 (column 0 the blank); labels: L >= 1 class ids.
    -> (nll, occ [T, V]): occ[t][c] = the posterior mass of the states that emit class c at frame t.  No path: (inf, zeros)."""
    labels = np.asarray(labels, np.int64)
    T, L = logp.shape[0], labels.shape[0]
    S = 2 * L + 1
    ext = np.zeros(S, np.int64)
    ext[1::2] = labels
    ok = (ext >= 0) & (ext < V)
    col = np.clip(ext, 0, V - 1)
    lp = np.where(ok[None, :], logp[:, col], -np.inf)                      # [T, S]
    skip = np.zeros(S, bool)                                               # state s = 2n+1 is entered from s - 2 iff labels[n] != labels[n-1]
    skip[3::2] = labels[1:] != labels[:-1]
    skip_from = _shift_up(skip.astype(np.float64), 2) > 0                  # state s leaves to s + 2
    alpha = np.full((T, S), -np.inf, dtype=lp.dtype)
    alpha[0, :2] = lp[0, :2]
    for t in range(1, T):
        a = alpha[t - 1]
        alpha[t] = _lse(a, _shift_down(a, 1), np.where(skip, _shift_down(a, 2), -np.inf)) + lp[t]
    beta = np.full((T, S), -np.inf, dtype=lp.dtype)
    beta[T - 1, S - 2:] = lp[T - 1, S - 2:]
    for t in range(T - 2, -1, -1):
        b = beta[t + 1]
        beta[t] = _lse(b, _shift_up(b, 1), np.where(skip_from, _shift_up(b, 2), -np.inf)) + lp[t]
    ll = float(_lse(alpha[T - 1, S - 1:], alpha[T - 1, S - 2: S - 1])[0])
    if not math.isfinite(ll):
        return math.inf, np.zeros((T, V))
    with np.errstate(invalid="ignore"):
        gamma = np.where(np.isfinite(lp), np.exp(alpha + beta - lp - ll), 0.0)     # alpha and beta both hold lp_t(s) once
    onehot = np.zeros((S, V))
    onehot[np.arange(S)[ok], col[ok]] = 1.0
    return -ll, gamma @ onehot


# ---- the whole entry ----------------------------------------------------------------------------------------------------------------

def _frame_terms(x, fl, V, f32):
    """-> (word CE, silence BCE, d(CE + BCE)/dx [B, T, V+1]) in float64; f32: the terms and their gradient by torch in float32."""
    B, T = fl.shape
    valid = (fl >= 1) & (fl < V)
    n = int(valid.sum())
    y = (fl == -100)
    if f32:
        xr = x.float().clone().requires_grad_(True)
        bce = F.binary_cross_entropy_with_logits(xr[..., V], y.float())
        ce = None
        if n > 0:
            tgt = torch.where(valid, fl.long() - 1, torch.full_like(fl.long(), -100))
            ce = F.cross_entropy(xr[..., 1:V].reshape(B * T, V - 1), tgt.reshape(-1), ignore_index=-100)
        (bce if ce is None else bce + ce).backward()
        return (math.nan if ce is None else float(ce.detach().double())), float(bce.detach().double()), xr.grad.double()
    d = torch.zeros(B, T, V + 1, dtype=torch.float64)
    logp = torch.log_softmax(x[..., 1:V], dim=-1)                           # columns 1..V-1: class k sits in column k
    ce = math.nan
    if n > 0:
        idx = (fl.long().clamp(1, V - 1) - 1).unsqueeze(-1)
        ce = float(-(logp.gather(-1, idx)[..., 0] * valid).sum() / n)
        onehot = torch.zeros_like(logp).scatter_(-1, idx, 1.0)
        d[..., 1:V] = (logp.exp() - onehot) * valid.unsqueeze(-1) / n
    xs = x[..., V]
    bce = float((F.softplus(xs) - xs * y).mean())                           # -[y log sigmoid(x) + (1 - y) log(1 - sigmoid(x))]
    d[..., V] = (torch.sigmoid(xs) - y.double()) / (B * T)
    return ce, bce, d


def _ctc_terms(x, labels, n_labels, V, f32):
    """-> (mean_b nll_b / L_b, nll [B], d/dx [B, T, V+1]) in float64; f32: the rows' log-softmax by torch in float32, cast to double."""
    B, T = x.shape[:2]
    logp = (torch.log_softmax(x[..., :V].float(), dim=-1).double() if f32 else torch.log_softmax(x[..., :V], dim=-1)).numpy()
    nll = torch.zeros(B, dtype=torch.float64)
    d = torch.zeros(B, T, V + 1, dtype=torch.float64)
    total = 0.0
    for b in range(B):
        L = int(n_labels[b])
        if L <= 0:
            continue
        nll_b, occ = ctc_clip(logp[b], labels[b, :L].numpy(), V)
        nll[b] = nll_b
        total += nll_b / L
        if math.isfinite(nll_b):
            d[b, :, :V] = torch.from_numpy((np.exp(logp[b]) - occ) / (B * L))
    return total / B, nll, d


def _parts(logits, frame_labels, labels, n_labels, V, f32):
    x = logits.double()[..., : V + 1]
    out = {}
    if frame_labels is not None:
        out["ce"] = _frame_terms(x, frame_labels, V, f32)
    if labels is not None:
        out["ctc"] = _ctc_terms(x, labels, n_labels, V, f32)
    return out


def _combine(parts, shape, scale, use_ce, use_ctc, f32):
    scale = float(torch.tensor(scale, dtype=torch.float32))                 # crosses the C ABI as a float
    losses = torch.full((3,), math.nan, dtype=torch.float64)
    nll = torch.zeros(shape[0], dtype=torch.float64)
    d = torch.zeros(shape, dtype=torch.float64)
    if use_ce:
        losses[0], losses[1] = parts["ce"][0], parts["ce"][1]
        d = d + parts["ce"][2]
    if use_ctc:
        losses[2], nll = parts["ctc"][0], parts["ctc"][1]
        d = d + parts["ctc"][2]
    d = scale * d
    if f32:
        losses, d = losses.float().double(), d.float().double()
    return losses, nll, d


def losses_and_grad(logits, frame_labels, labels, n_labels, V, scale, use_ce, use_ctc):
    """The header's contract in float64: logits [B, T, >= V+1], frame_labels [B, T] int, labels [B, >= max L] int, n_labels [B] int.
    -> (losses [3] (NaN where not requested), nll [B], dlogits [B, T, V+1] = scale * d(requested losses) / d logits)."""
    parts = _parts(logits, frame_labels if use_ce else None, labels if use_ctc else None, n_labels, V, False)
    return _combine(parts, (logits.shape[0], logits.shape[1], V + 1), scale, use_ce, use_ctc, False)


def e32(logits, frame_labels, labels, n_labels, V, scale, use_ce, use_ctc):
    """The same with float32 row normalisers (module docstring): the yardstick E32 = error of this against losses_and_grad."""
    parts = _parts(logits, frame_labels if use_ce else None, labels if use_ctc else None, n_labels, V, True)
    return _combine(parts, (logits.shape[0], logits.shape[1], V + 1), scale, use_ce, use_ctc, True)


# ---- the case table -----------------------------------------------------------------------------------------------------------------

def _rand_labels(seed, L, V):
    """L class ids in 1..V-1 without equal neighbours, then one planted pair of equal neighbours (positions 1, 2; from L = 4 on) and the
    first class again at the last position (from L = 5 on): a class that repeats at a distance."""
    rs = np.random.RandomState(seed)
    lab = [int(rs.randint(1, V))]
    while len(lab) < L:
        c = int(rs.randint(1, V))
        if c != lab[-1]:
            lab.append(c)
    if L >= 4:
        lab[2] = lab[1]
        if lab[3] == lab[2]:
            lab[3] = 1 + lab[2] % (V - 1)
    if L >= 5 and lab[L - 2] != lab[0]:
        lab[L - 1] = lab[0]
    return lab


def repeats(lab):
    return sum(1 for a, b in zip(lab[1:], lab[:-1]) if a == b)


CASES = {}


def _add(name, T, V, labels, logits="normal", frames="mixed", max_labels=None):
    assert name not in CASES
    CASES[name] = dict(name=name, T=T, V=V, labels=[list(l) for l in labels], logits=logits, frames=frames,
                       max_labels=max_labels or max(1, max(len(l) for l in labels)))


# 1. every lattice kernel at both ends of its label range (S = 2 L + 1 states): one wave up to 64, <128>, <256>, <512>, <1024>
for _name, _T, _V, _Ls in (("wave63_beside_1", 40, 37, (31, 1)), ("wg128_first", 48, 40, (32,)), ("wg128_last", 80, 40, (63,)),
                           ("wg256_first", 80, 40, (64,)), ("wg256_last", 140, 40, (127,)), ("wg512_first", 140, 40, (128,)),
                           ("wg512_last", 270, 40, (255,)), ("wg1024_first_beside_3", 270, 40, (256, 3)),
                           ("wg1024_last_beside_3", 530, 40, (511, 3))):
    _add(_name, _T, _V, [_rand_labels(_T + _L, _L, _V) for _L in _Ls])

# 2. frame counts: on the one-wave kernel and again in a launch of <128> (max_labels = 32)
_TIGHT = [1, 1, 3, 4, 4, 4, 2]                                                # 7 labels + 3 adjacent repeats: 10 frames, one path
for _wide in (None, 32):
    _sfx = "" if _wide is None else "_wide32"
    _add("T1_L1" + _sfx, 1, 6, [[3]], max_labels=_wide)
    _add("T2" + _sfx, 2, 6, [[3], [2, 4]], max_labels=_wide)
    for _T in (8, 9, 10, 17):                                                 # the one-wave kernel's prefetch blocks of 8 start at t = 1
        _add(f"T{_T}_L3" + _sfx, _T, 6, [[2, 5, 1]], max_labels=_wide)
    _add("tight" + _sfx, len(_TIGHT) + repeats(_TIGHT), 6, [_TIGHT], max_labels=_wide)
    _add("infeasible_beside_feasible" + _sfx, len(_TIGHT) + repeats(_TIGHT) - 1, 6, [_TIGHT, [5, 2]], max_labels=_wide)
_L40 = _rand_labels(40, 40, 64)
_add("tight_L40", 40 + repeats(_L40), 64, [_L40])

# 3. label patterns
_add("adjacent_repeats", 24, 12, [[3, 3, 5, 5, 7]])
_add("run_of_three", 24, 12, [[4, 4, 4, 2]])
_add("all_equal", 24, 12, [[6] * 5])
_add("distant_same_class", 24, 12, [[3, 5, 3, 8, 3]])
_add("empty_between_feasible", 24, 12, [[4, 1, 7, 2], [], [9, 9, 3]])
_add("label_class_V_and_negative", 24, 12, [[3, 12, 5], [2, 4], [5, -1]])

# 4. the 256-column loops of the row kernels
for _V in (3, 4, 257, 258, 600):
    _add(f"V{_V}", 12, _V, [[1, 2] if _V == 3 else [_V - 1, 1], [2, 1]])

# 5. logit patterns
LOGIT_SHAPES = [(40, 5, 6), (96, 64, 40), (48, 258, 8)]
LOGIT_PATTERNS = ["normal", "plus1e4", "minus1e4", "blank_spike", "label_spike", "equal_row", "silence_levels"]
OFFSET_CASES = []
for _T, _V, _L in LOGIT_SHAPES:
    for _p in LOGIT_PATTERNS:
        _add(f"logits_{_p}_T{_T}_V{_V}_L{_L}", _T, _V, [_rand_labels(_T + _V, _L, _V)], logits=_p)
        if _p in ("plus1e4", "minus1e4"):
            OFFSET_CASES.append(f"logits_{_p}_T{_T}_V{_V}_L{_L}")

# 6. frame labels
_add("frames_all_ignored", 12, 6, [[2, 4]], frames="all_ignored")
_add("frames_0_and_V", 12, 6, [[2, 4]], frames="zero_and_V")

CASE_NAMES = list(CASES)


def clip_state(case, b):
    """'empty', 'infeasible' or 'ok' for clip b of a case (from the labels and the frame count alone)."""
    lab = case["labels"][b]
    if not lab:
        return "empty"
    if any(c < 0 or c >= case["V"] for c in lab) or case["T"] < len(lab) + repeats(lab):
        return "infeasible"
    return "ok"


def is_special(case):
    """A case torch does not define: an empty or infeasible clip, or no frame with a label."""
    return case["frames"] == "all_ignored" or any(clip_state(case, b) != "ok" for b in range(len(case["labels"])))


_MADE = {}


def make(name):
    """-> dict(x float32 [B, T, V+1], fl int32 [B, T], labels int32 [B, max_labels], n_labels int32 [B], + the case's fields).
    Seeded by the name's position in the table; computed once and shared (not to be modified)."""
    if name in _MADE:
        return _MADE[name]
    case = CASES[name]
    T, V, B = case["T"], case["V"], len(case["labels"])
    g = torch.Generator().manual_seed(1000 + CASE_NAMES.index(name))
    x = torch.randn(B, T, V + 1, generator=g) * 2
    first = [lab[0] if lab else 1 for lab in case["labels"]]
    p = case["logits"]
    if p == "plus1e4":
        x[..., :V] += 1e4                                                   # the silence column stays
    elif p == "minus1e4":
        x[..., :V] -= 1e4
    elif p == "blank_spike":
        x[:, ::3, 0] = x[:, ::3, 1:V].amax(-1) + 90.0                       # exp(m1 - m0) underflows: the blank is the whole row
    elif p == "label_spike":
        for b in range(B):
            x[b, ::5, first[b]] += 80.0
    elif p == "equal_row":
        x[:, min(3, T - 1), :] = 1.5
    elif p == "silence_levels":
        x[..., V] = torch.tensor([-30.0, 0.0, 30.0]).repeat(T // 3 + 1)[:T]
    else:
        assert p == "normal", p
    fl = torch.randint(1, V, (B, T), generator=g, dtype=torch.int32)
    fl[torch.rand(B, T, generator=g) < 0.4] = -100
    f = case["frames"]
    if f == "all_ignored":
        fl[:] = -100
    else:
        fl[:, 0] = V - 1                                                    # a labelled frame and (from T = 2 on) a silent one in every clip
        if T >= 2:
            fl[:, T - 1] = -100
        if f == "zero_and_V":
            fl[:, 1], fl[:, 2], fl[:, 3] = 0, V, V + 3
    Lmax = case["max_labels"]
    labels = torch.zeros(B, Lmax, dtype=torch.int32)
    for b, lab in enumerate(case["labels"]):
        labels[b, : len(lab)] = torch.tensor(lab, dtype=torch.int32)
    n_labels = torch.tensor([len(lab) for lab in case["labels"]], dtype=torch.int32)
    out = dict(case, B=B, x=x, fl=fl, lab=labels, n_labels=n_labels, special=is_special(case))
    _MADE[name] = out
    return out


_REF = {}


def reference(name, mode):
    """-> ((losses, nll, dlogits) of losses_and_grad, the same of e32) for a case under MODES[mode]; both lattices run once per case."""
    c = make(name)
    if name not in _REF:
        _REF[name] = tuple(_parts(c["x"], c["fl"], c["lab"], c["n_labels"], c["V"], f32) for f32 in (False, True))
    use_ce, use_ctc, scale = MODES[mode]
    shape = (c["B"], c["T"], c["V"] + 1)
    return tuple(_combine(_REF[name][i], shape, scale, use_ce, use_ctc, bool(i)) for i in (0, 1))
