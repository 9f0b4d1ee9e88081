"""Plain restatement of the emission head's contract (include/lyricalign.h: la_fc_emissions, la_fc_emissions_x2, la_emissions_from_logits),
importable without a GPU.

Like tests/row_kernel_reference.py, every function computes in the dtype of its floating inputs: handed float64 tensors it is the reference
the GPU tests compare against; handed the same inputs in float32 it is the CPU float32 evaluation whose error against the float64 result
is the yardstick E32.  Nothing here follows the kernels' structure (no strips, no partial (max, sum) pairs, no gather): Linear, then
torch.log_softmax over the variant's column range, then the reference's emission formulas in their naive order.  It is pinned to
oracle/model_oracle.py and to the reference's own recorded output by tests/test_host_head_kernels.py.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from row_kernel_reference import rel_err  # noqa: F401  (the metric of the measured group, re-exported)

PLAIN, CTC = 0, 1
CLAMP = -1000.0


def logits(act: torch.Tensor, w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """Linear(2H -> V): act [rows][K], w [V][K], bias [V] -> [rows][V]"""
    return act @ w.T + bias


def norm_range(vocab: int, variant: int):
    """Inclusive column range of the normaliser, which is also the range of valid class ids' upper end: (lo, hi)."""
    return (1, vocab - 2) if variant == CTC else (0, vocab - 1)


def log_softmax_part(lg: torch.Tensor, variant: int) -> torch.Tensor:
    """[..., V] -> [..., V]: log-softmax over the normaliser's columns; the columns outside it hold NaN (nothing may read them)."""
    V = lg.shape[-1]
    lo, hi = norm_range(V, variant)
    out = torch.full_like(lg, math.nan)
    out[..., lo:hi + 1] = torch.log_softmax(lg[..., lo:hi + 1], dim=-1)
    return out


def silence_terms(x0: torch.Tensor):
    """The reference's naive order: sil = sigmoid(x0); (log(sil), log(1 - sil)), either may be -inf."""
    sil = torch.sigmoid(x0)
    return torch.log(sil), torch.log(1.0 - sil)


def parts(lg: torch.Tensor, variant: int):
    """lg [B][T][V] -> (lsm [B][T][V], log_sil [B][T] or None, log_voiced [B][T] or None): everything of `emissions` that does not
    depend on the labels (a test that runs one set of logits with several label sets evaluates it once)."""
    lsm = log_softmax_part(lg, variant)
    if variant == CTC:
        return (lsm,) + silence_terms(lg[..., lg.shape[-1] - 1])
    return lsm, None, None


def emissions(lg: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, max_labels: int, variant: int) -> torch.Tensor:
    """lg [B][T][V], labels [B][>= max_labels] (any integers), n_labels [B] -> the compact layout [B][T][1 + max_labels].
    Column 0: CTC max(log sigmoid(x[V-1]), -1000); plain max(lsm[0], -1000).  Column 1 + n, n < min(n_labels, max_labels): -1000 for a
    class id outside 1..hi, else max(lsm[c] (+ log(1 - sil) for CTC), -1000).  Columns past that are NOT WRITTEN and hold NaN here."""
    return compact(*parts(lg, variant), labels, n_labels, max_labels, variant)


def compact(lsm, log_sil, log_voiced, labels: torch.Tensor, n_labels: torch.Tensor, max_labels: int, variant: int) -> torch.Tensor:
    B, T, V = lsm.shape
    _, hi = norm_range(V, variant)
    clamp = torch.tensor(CLAMP, dtype=lsm.dtype)
    em = torch.full((B, T, 1 + max_labels), math.nan, dtype=lsm.dtype)
    if variant == CTC:
        em[..., 0] = torch.maximum(log_sil, clamp)
    else:
        log_voiced = torch.zeros(B, T, dtype=lsm.dtype)
        em[..., 0] = torch.maximum(lsm[..., 0], clamp)
    for b in range(B):
        L = min(max(int(n_labels[b]), 0), max_labels)
        for n in range(L):
            c = int(labels[b, n])
            if 1 <= c <= hi:
                em[b, :, 1 + n] = torch.maximum(lsm[b, :, c] + log_voiced[b], clamp)
            else:
                em[b, :, 1 + n] = clamp
    return em


def written(n_labels: torch.Tensor, max_labels: int) -> torch.Tensor:
    """[B][1 + max_labels] bool: the columns of the compact layout an entry writes for each clip."""
    L = n_labels.long().clamp(0, max_labels)
    return torch.arange(1 + max_labels).unsqueeze(0) <= L.unsqueeze(1)


def x2_domain(rows: int, in_dim: int, vocab: int) -> bool:
    """Where la_fc_emissions_x2 runs the normaliser product on the f16 pipe (the header: in_dim % 128, >= 192 tiles of 256 x 256)."""
    return in_dim % 128 == 0 and in_dim >= 256 and -(-rows // 256) * -(-vocab // 256) >= 192


def workspace_layout(batch: int, frames: int, in_dim: int, vocab: int, max_labels: int, elem_size: int, x2: bool = False) -> dict:
    """The parts of the head's workspace in order, each rounded up to 256 bytes: gathered weight rows, their biases, the raw logits of the
    gathered columns, one (max, sum) float pair per row and 64-column strip of whole 256-column tiles, and for x2 the planes of act and
    their scales.  -> {part: (offset, bytes)} and "total".  Pinned to the library's queries by the host test; the GPU test uses the
    offset of "partials" to see which strips a call wrote."""
    up = lambda n: (n + 255) // 256 * 256
    rows, S = batch * frames, max_labels + 1
    parts = [("wg", batch * S * in_dim * elem_size), ("bg", batch * S * 4), ("raw", rows * S * 4), ("partials", rows * 4 * -(-vocab // 256) * 8)]
    if x2:
        parts += [("planes", rows * 2 * in_dim * 2), ("inv", rows * 4)]
    out, o = {}, 0
    for name, n in parts:
        out[name] = (o, n)
        o += up(n)
    out["total"] = o
    return out


# ---- the silence terms of a float32 device, bracketed ------------------------------------------------------------------------------

def sweep_values() -> torch.Tensor:
    """The silence logits of the sweep, all of at most 8 significant bits (exact in bf16, f16 and the f16x2 planes): k/4 for |k| <= 128,
    the integers -104 .. 40, and 16.5, 16.75, 17, 17.5, -87, -89 -- without the open interval (-89, -87), where the float32 sigmoid is
    subnormal and the result depends on the flush mode (so the integer -88 is not among them)."""
    v = [k / 4 for k in range(-128, 129)] + [float(i) for i in range(-104, 41)] + [16.5, 16.75, 17.0, 17.5, -87.0, -89.0]
    v = sorted({x for x in v if not -89.0 < x < -87.0})
    t = torch.tensor(v, dtype=torch.float32)
    assert torch.equal(t.to(torch.bfloat16).float(), t)
    return t


def _ulp32(v: float) -> float:
    return float(np.spacing(np.float32(abs(v)))) if math.isfinite(v) else 0.0


def _log64(v) -> float:
    v = float(v)
    return math.log(v) if v > 0.0 else -math.inf


def silence_bracket(x0: float):
    """x0: an exactly known float32 silence logit -> ((lo, hi) for max(log sil, -1000), (lo, hi) for max(log(1 - sil), -1000), saturated).
    The five float32 values nearest sigmoid(x0) in float64 (the rounded value and two neighbours on each side, clipped to [0, 1]); for
    each, log(s) and log(float32(1 - s)) in float64; the minimum and the maximum, each widened by 4 float32 ulps of itself; -inf -> -1000.
    saturated: every candidate gives 1 - s == 0 (the label columns are then exactly -1000)."""
    x = float(np.float32(x0))
    s64 = 1.0 / (1.0 + math.exp(-x)) if x >= 0 else math.exp(x) / (1.0 + math.exp(x))
    mid = np.float32(s64)
    cand = [mid]
    up = dn = mid
    for _ in range(2):
        up = np.nextafter(up, np.float32(2.0), dtype=np.float32)
        dn = np.nextafter(dn, np.float32(-1.0), dtype=np.float32)
        cand += [up, dn]
    cand = [np.float32(min(max(float(c), 0.0), 1.0)) for c in cand]
    log_s = [_log64(c) for c in cand]
    one_minus = [np.float32(np.float32(1.0) - c) for c in cand]
    log_v = [_log64(c) for c in one_minus]

    def interval(vals):
        lo, hi = min(vals), max(vals)
        lo = CLAMP if lo == -math.inf else max(lo - 4 * _ulp32(lo), CLAMP)
        hi = CLAMP if hi == -math.inf else max(hi + 4 * _ulp32(hi), CLAMP)
        return lo, hi

    return interval(log_s), interval(log_v), all(float(c) == 0.0 for c in one_minus)
