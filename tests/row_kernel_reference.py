"""Plain restatements of the small row kernels of the training and decoding paths (include/lyricalign.h), importable without a GPU.

Every function is a handful of torch ops that computes in the dtype of its floating inputs: handed float64 tensors it is the reference
the GPU tests compare against; handed the same inputs in float32 it is the CPU float32 evaluation whose error against the float64 result
is the yardstick E32 of those tests.  Nothing here follows the kernels' loop structure: each is written from the header's statement of
the operation and pinned to an independent yardstick (float64 autograd, F.cross_entropy, torch.optim.AdamW,
scipy.signal.resample_poly) by tests/test_host_row_kernels.py.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

LN_EPS = 1e-5


def rel_err(a: torch.Tensor, ref: torch.Tensor) -> float:
    """max |a - ref| / max(|ref|, 1) with ref in float64: the error metric of the measured group."""
    a, ref = a.detach().double().reshape(-1), ref.detach().double().reshape(-1)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if a.numel() == 0:
        return 0.0
    return float(((a - ref).abs() / ref.abs().clamp_min(1.0)).max())


# ---- decoding rows ------------------------------------------------------------------------------------------------------------------

def stable_topk(x: torch.Tensor, k: int):
    """The k largest of each row with the LOWEST index first among equals, and the row's log-sum-exp in float64.
    (torch.topk does not promise an order among ties; a stable descending sort does.)"""
    vals, idx = torch.sort(x, dim=1, descending=True, stable=True)
    return vals[:, :k].contiguous(), idx[:, :k].contiguous(), torch.logsumexp(x.double(), 1)


def argmax_rows(x: torch.Tensor) -> torch.Tensor:
    """Index of the first maximum of each row (0 for a row of equal values, -inf included)."""
    return stable_topk(x, 1)[1][:, 0]


def embed_tokens(tokens: torch.Tensor, emb: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """x[b][i] = emb[clamp(tokens[b][i], 0, n_vocab - 1)] + pos[i]"""
    return emb[tokens.clamp(0, emb.shape[0] - 1)] + pos[: tokens.shape[1]].unsqueeze(0)


def embed_tokens_bwd(dx: torch.Tensor, tokens: torch.Tensor, n_vocab: int):
    """dx [B][n][d] -> (dtok [n_vocab][d]: rows of dx added to the row of their clamped token, dpos [n][d] = sum over b ascending)."""
    B, n, d = dx.shape
    dtok = torch.zeros(n_vocab, d, dtype=dx.dtype)
    dtok.index_add_(0, tokens.clamp(0, n_vocab - 1).reshape(-1), dx.reshape(B * n, d))
    dpos = dx[0].clone()
    for b in range(1, B):
        dpos = dpos + dx[b]
    return dtok, dpos


def embed_tokens_bwd_abs(dx: torch.Tensor, tokens: torch.Tensor, n_vocab: int):
    """Per element of dtok: (sum of |g| over its contributions, their count c) -- the terms of the derived atomic-order bound."""
    B, n, d = dx.shape
    flat = tokens.clamp(0, n_vocab - 1).reshape(-1)
    sabs = torch.zeros(n_vocab, d, dtype=torch.float64)
    sabs.index_add_(0, flat, dx.double().abs().reshape(B * n, d))
    cnt = torch.bincount(flat, minlength=n_vocab).double().unsqueeze(1)
    return sabs, cnt


# ---- elementwise --------------------------------------------------------------------------------------------------------------------

def mish(x):
    return F.mish(x)


def mish_bwd(x, dy):
    """dy * d/dx [x tanh(softplus(x))] = dy * (tanh(sp) + x (1 - tanh(sp)^2) sigmoid(x))"""
    th = torch.tanh(F.softplus(x))
    return dy * (th + x * (1 - th * th) * torch.sigmoid(x))


def gelu(x):
    return F.gelu(x)          # the exact (erf) form: whisper's nn.GELU


def gelu_bwd(x, dy):
    """dy * (Phi(x) + x phi(x))"""
    cdf = 0.5 * (1 + torch.erf(x * (1 / math.sqrt(2))))
    pdf = torch.exp(-0.5 * x * x) * (1 / math.sqrt(2 * math.pi))
    return dy * (cdf + x * pdf)


def add(a, b):
    return a + b


def scale(x, alpha: float):
    return x * torch.tensor(alpha, dtype=torch.float32).to(x.dtype)      # alpha crosses the C ABI as a float


def mask_scale(x, mask, s: float):
    return torch.where(mask != 0, x * torch.tensor(s, dtype=torch.float32).to(x.dtype), torch.zeros_like(x))


# ---- optimizer ----------------------------------------------------------------------------------------------------------------------

def grad_sqnorm(g) -> float:
    return float((g.double() ** 2).sum())


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, wd, step, clip_sum_sq, max_norm, grad_prescale):
    """The header's formula: g' = g prescale min(1, max_norm / (sqrt(sum_sq) prescale + 1e-6)); decoupled decay; bias-corrected Adam.
    The float scalars cross the C ABI as float32, so they are rounded to float32 first.  Returns (p, m, v)."""
    f32 = lambda s: float(torch.tensor(s, dtype=torch.float32))
    lr, beta1, beta2, eps, wd, max_norm, grad_prescale = map(f32, (lr, beta1, beta2, eps, wd, max_norm, grad_prescale))
    clip = 1.0
    if clip_sum_sq is not None:
        clip = min(1.0, max_norm / (math.sqrt(clip_sum_sq) * grad_prescale + 1e-6))
    gs = g * (clip * grad_prescale)
    p = p * (1 - lr * wd)
    m = beta1 * m + (1 - beta1) * gs
    v = beta2 * v + (1 - beta2) * gs * gs
    p = p - (lr / (1 - beta1 ** step)) * (m / (v.sqrt() / math.sqrt(1 - beta2 ** step) + eps))
    return p, m, v


# ---- layout -------------------------------------------------------------------------------------------------------------------------

def transpose_pad(x: torch.Tensor, out_rows: int, out_cols: int) -> torch.Tensor:
    """x [..., rows, cols] -> [..., out_rows, out_cols]: the transpose in the top-left corner, zeros elsewhere."""
    rows, cols = x.shape[-2:]
    out = torch.zeros(*x.shape[:-2], out_rows, out_cols, dtype=x.dtype)
    out[..., :cols, :rows] = x.transpose(-1, -2)
    return out


def col2im3(dcols: torch.Tensor, stride: int, rows_out: int) -> torch.Tensor:
    """dcols [B][T_out][3][C] -> out [B][rows_out][C]: out[b][t stride + tap] += dcols[b][t][tap]; per element the taps are added
    in the order 0, 1, 2 (at most one t per tap reaches a row)."""
    B, T, _, C = dcols.shape
    out = torch.zeros(B, rows_out, C, dtype=dcols.dtype)
    for tap in range(3):
        rows = torch.arange(T) * stride + tap
        out[:, rows] = out[:, rows] + dcols[:, :, tap]
    return out


# ---- softmax rows -------------------------------------------------------------------------------------------------------------------

def causal_visible(rows: int, cols: int, causal_q_len: int) -> torch.Tensor:
    """[rows][cols] bool: row r is query i = r mod q_len and sees keys 0 .. i + cols - q_len; a query that would see no key
    (cols < q_len) sees key 0."""
    if causal_q_len <= 0:
        return torch.ones(rows, cols, dtype=torch.bool)
    i = torch.arange(rows) % causal_q_len
    last = (i + cols - causal_q_len).clamp(0, cols - 1)
    return torch.arange(cols).unsqueeze(0) <= last.unsqueeze(1)


def softmax_rows(s: torch.Tensor, causal_q_len: int = 0) -> torch.Tensor:
    vis = causal_visible(s.shape[0], s.shape[1], causal_q_len)
    p = torch.softmax(s.masked_fill(~vis, float("-inf")), dim=1)
    return torch.where(vis, p, torch.zeros_like(p))


def softmax_bwd_rows(p: torch.Tensor, dp: torch.Tensor) -> torch.Tensor:
    """dS = P (dP - sum_c dP P)"""
    return p * (dp - (dp * p).sum(1, keepdim=True))


# ---- LayerNorm backward -------------------------------------------------------------------------------------------------------------

def layernorm_bwd(x, dy, gamma, residual=None):
    """-> dx (+ residual), dy * xhat, dgamma, dbeta for y = LayerNorm(x) gamma + beta, eps 1e-5, biased variance."""
    mean = x.mean(1, keepdim=True)
    xc = x - mean
    rstd = 1 / torch.sqrt((xc * xc).mean(1, keepdim=True) + LN_EPS)
    xhat = xc * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    if residual is not None:
        dx = residual + dx
    dy_xhat = dy * xhat
    return dx, dy_xhat, dy_xhat.sum(0), dy.sum(0)


# ---- cross entropy ------------------------------------------------------------------------------------------------------------------

def cross_entropy(logits: torch.Tensor, target: torch.Tensor, scale_: float):
    """F.cross_entropy(ignore_index=-100, 'mean') where every target outside [0, V) counts as ignored.
    -> (loss (nan if nothing counts), 1/count (0 then), scale * dloss/dlogits)"""
    R, V = logits.shape
    ok = (target >= 0) & (target < V)
    cnt = int(ok.sum())
    logp = torch.log_softmax(logits, dim=1)
    picked = logp.gather(1, target.clamp(0, V - 1).unsqueeze(1))[:, 0]
    if cnt == 0:
        return float("nan"), 0.0, torch.zeros_like(logits)
    loss = -(picked * ok).sum() / cnt
    onehot = torch.zeros_like(logits).scatter_(1, target.clamp(0, V - 1).unsqueeze(1), 1.0)
    grad = (logp.exp() - onehot) * ok.unsqueeze(1) * (float(torch.tensor(scale_, dtype=torch.float32)) / cnt)
    return loss, 1.0 / cnt, grad


# ---- attention statistics -----------------------------------------------------------------------------------------------------------

def attention_bwd_stats(q, k, o, dout, B: int, Tq: int, Tk: int, H: int, causal: bool):
    """q / o / dout [B*Tq][H*64], k [B*Tk][H*64] (q pre-scaled) -> lse [B][H][Tq] = log sum_j exp(q_i . k_j) over visible keys
    (causal: j <= i), dvec [B][H][Tq] = sum_d dout o."""
    qh = q.reshape(B, Tq, H, 64).permute(0, 2, 1, 3)
    kh = k.reshape(B, Tk, H, 64).permute(0, 2, 1, 3)
    s = qh @ kh.transpose(-1, -2)
    if causal:
        s = s.masked_fill(torch.arange(Tk).unsqueeze(0) > torch.arange(Tq).unsqueeze(1), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    dvec = (o * dout).reshape(B, Tq, H, 64).sum(-1).permute(0, 2, 1)
    return lse, dvec


# ---- polyphase resampling -----------------------------------------------------------------------------------------------------------

# (sample rate, input length): up > down (8, 11.025, 12 kHz), down > up, and inputs shorter than the filter
RESAMPLE_CASES = [(8000, 1), (8000, 7), (8000, 4001), (11025, 5000), (12000, 3333), (32000, 5), (96000, 1234), (44100, 3)]


def resample_input(sr: int, n_in: int) -> np.ndarray:
    """float64, uniform in [-1, 1): the same signal for the host and the GPU test of one case"""
    return np.random.RandomState(sr + n_in).uniform(-1.0, 1.0, n_in)


def resample_poly(x: torch.Tensor, up: int, down: int, h: torch.Tensor, skip: int, n_out: int) -> torch.Tensor:
    """y[n] = sum_k h[(n + skip) down - k up] x[k], n < n_out, the sum over every k in [0, n_in) whose tap index lies in [0, len h):
    the header's formula term by term (zero-stuffing by `up`, FIR, keep every `down`-th sample, drop `skip`), one gather per tap."""
    n_in, h_len = x.shape[0], h.shape[0]
    h = h.to(x.dtype)
    pos = (torch.arange(n_out, dtype=torch.int64) + skip) * down
    k_top = pos // up                                    # the largest k with a non-negative tap index
    y = torch.zeros(n_out, dtype=x.dtype)
    for t in range((h_len + up - 1) // up + 1):
        k = k_top - t
        j = pos - k * up
        ok = (k >= 0) & (k < n_in) & (j >= 0) & (j < h_len)
        y = y + torch.where(ok, h[j.clamp(0, h_len - 1)] * x[k.clamp(0, n_in - 1)], torch.zeros_like(y))
    return y
