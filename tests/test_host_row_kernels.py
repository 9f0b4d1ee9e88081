"""The float64 restatements of tests/row_kernel_reference.py pinned to independent yardsticks, and the host-side argument checks of the
row kernels' entry points.  Runs without a GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import row_kernel_reference as R
from row_kernel_reference import RESAMPLE_CASES, resample_input

TIGHT = 1e-12          # two float64 evaluations of the same few-term formula


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, tol=TIGHT):
    assert R.rel_err(a, b) <= tol, R.rel_err(a, b)


@pytest.mark.parametrize("M,d", [(1, 4), (5, 256), (37, 320)])
def test_layernorm_backward_restatement_matches_autograd(M, d):
    g = _g(M + d)
    x = (torch.randn(M, d, generator=g) * torch.exp(torch.randn(M, 1, generator=g))).double()
    dy, res, gamma = torch.randn(M, d, generator=g).double(), torch.randn(M, d, generator=g).double(), (torch.rand(d, generator=g) + 0.5).double()
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), torch.zeros(d, dtype=torch.float64, requires_grad=True)
    F.layer_norm(xr, (d,), gr, br, 1e-5).backward(dy)
    dx, dy_xhat, dgamma, dbeta = R.layernorm_bwd(x, dy, gamma, res)
    _close(dx, xr.grad + res, 1e-11)
    _close(dgamma, gr.grad, 1e-11)
    _close(dbeta, br.grad)
    _close(dy_xhat.sum(0), gr.grad, 1e-11)
    _close(R.layernorm_bwd(x, dy, gamma)[0], xr.grad, 1e-11)


def test_elementwise_derivative_restatements_match_autograd():
    x = torch.cat([torch.randn(4000, generator=_g(1)).double() * 3, torch.linspace(-30, 30, 2401, dtype=torch.float64),
                   torch.tensor([-100.0, -88.0, -20.0, 0.0, 19.999, 20.0, 20.001, 88.0], dtype=torch.float64)])
    dy = torch.randn(x.shape, generator=_g(2)).double()
    for fwd, bwd in ((F.mish, R.mish_bwd), (F.gelu, R.gelu_bwd)):
        xr = x.clone().requires_grad_(True)
        fwd(xr).backward(dy)
        _close(bwd(x, dy), xr.grad, 1e-13)
    _close(R.mish(x), x * torch.tanh(F.softplus(x)), 1e-15)
    _close(R.gelu(x), 0.5 * x * (1 + torch.erf(x / math.sqrt(2))), 1e-15)


@pytest.mark.parametrize("rows,cols,q_len", [(3, 65, 0), (10, 5, 5), (6, 10, 3), (2, 9, 1)])
def test_softmax_restatements_match_autograd_and_the_causal_rule(rows, cols, q_len):
    s = (torch.randn(rows, cols, generator=_g(rows * cols)) * 4).double()
    dp = torch.randn(rows, cols, generator=_g(7)).double()
    vis = R.causal_visible(rows, cols, q_len)
    for r in range(rows):                  # the header's rule, spelled out: keys 0 .. (r mod q_len) + cols - q_len
        last = cols - 1 if q_len == 0 else (r % q_len) + cols - q_len
        assert vis[r].tolist() == [c <= last for c in range(cols)]
    sr = s.clone().requires_grad_(True)
    p_auto = torch.softmax(sr.masked_fill(~vis, float("-inf")), dim=1)
    p = R.softmax_rows(s, q_len)
    _close(p, p_auto)
    assert bool((p[~vis] == 0).all())
    _close(p.sum(1), torch.ones(rows, dtype=torch.float64), 1e-14)
    p_auto.backward(dp)
    _close(R.softmax_bwd_rows(p, dp), sr.grad, 1e-14)


def test_causal_query_without_a_visible_key_sees_key_0():
    vis = R.causal_visible(12, 3, 6)       # cols < q_len: queries 0, 1, 2 would see nothing
    assert [int(v.sum()) for v in vis] == [1, 1, 1, 1, 2, 3] * 2
    assert bool(vis[:, 0].all())


@pytest.mark.parametrize("rows,V", [(1, 1), (4, 5), (64, 257)])
def test_cross_entropy_restatement_matches_torch(rows, V):
    g = _g(rows + V)
    logits = (torch.randn(rows, V, generator=g) * 3).double()
    if rows > 2:
        logits[1] += 1e4
        logits[2] -= 1e4
    target = torch.randint(0, V, (rows,), generator=g)
    if rows > 3:
        target[3] = -100
    lr = logits.clone().requires_grad_(True)
    want = F.cross_entropy(lr, target, ignore_index=-100)
    want.backward()
    loss, inv_count, grad = R.cross_entropy(logits, target, 0.125)
    _close(loss, want)
    assert inv_count == 1.0 / int((target != -100).sum())
    _close(grad, 0.125 * lr.grad, 1e-15)
    if rows > 3:
        # a target of -5 or >= V is treated like -100 (the kernel's rule): the same numbers as torch with those rows ignored
        t2 = target.clone()
        t2[0], t2[rows - 1] = -5, V + 2
        t3 = torch.where((t2 < 0) | (t2 >= V), torch.full_like(t2, -100), t2)
        lr2 = logits.clone().requires_grad_(True)
        want2 = F.cross_entropy(lr2, t3, ignore_index=-100)
        want2.backward()
        loss2, inv2, grad2 = R.cross_entropy(logits, t2, 0.125)
        _close(loss2, want2)
        _close(grad2, 0.125 * lr2.grad, 1e-15)
        assert inv2 == 1.0 / int((t3 != -100).sum())
    loss0, inv0, grad0 = R.cross_entropy(logits, torch.full((rows,), -100), 0.125)
    assert math.isnan(loss0) and inv0 == 0.0 and bool((grad0 == 0).all())


@pytest.mark.parametrize("B,T,stride,C,rows_out", [(1, 1, 1, 1, 3), (2, 5, 1, 3, 7), (2, 5, 2, 3, 11), (1, 4, 2, 8, 12)])
def test_col2im3_restatement_is_the_gradient_of_column_extraction(B, T, stride, C, rows_out):
    g = _g(T * stride + C)
    dcols = torch.randn(B, T, 3, C, generator=g).double()
    inp = torch.randn(B, rows_out, C, generator=g).double().requires_grad_(True)
    # F.unfold-style extraction of the k = 3 windows: cols[b][t][tap] = inp[b][t stride + tap]
    cols = torch.stack([inp[:, tap: tap + (T - 1) * stride + 1: stride] for tap in range(3)], dim=2)
    assert cols.shape == dcols.shape
    unf = F.unfold(inp.detach().permute(0, 2, 1).unsqueeze(-1), kernel_size=(3, 1), stride=(stride, 1))      # [B][C*3][L]
    L = unf.shape[-1]
    assert L >= T
    assert torch.equal(unf.reshape(B, C, 3, L)[..., :T].permute(0, 3, 2, 1), cols.detach())
    (cols * dcols).sum().backward()
    _close(R.col2im3(dcols, stride, rows_out), inp.grad, 1e-15)


@pytest.mark.parametrize("sr,n_in", RESAMPLE_CASES)
def test_resampler_restatement_matches_scipy(sr, n_in):
    """The header's formula with the project's float32 filter table against scipy.signal.resample_poly in float64.  The only difference is
    the rounding of h to float32: |dy| <= 2^-24 max_phase sum |h| for |x| <= 1."""
    from scipy.signal import resample_poly
    from lyricalignment_amd.utils.audio import _design
    fr = Fraction(16000, sr)
    up, down = fr.numerator, fr.denominator
    h, skip = _design(up, down)
    x = resample_input(sr, n_in)
    want = resample_poly(x, up, down)
    n_out = int(math.ceil(n_in * up / down))
    assert want.shape[0] == n_out
    got = R.resample_poly(torch.from_numpy(x), up, down, torch.from_numpy(h), skip, n_out).numpy()
    bound = 2.0 ** -24 * max(np.abs(h[p::up].astype(np.float64)).sum() for p in range(up)) + 1e-12
    err = np.abs(got - want).max()
    print(f"resample_restatement sr={sr} n={n_in} err={err:.3e} bound={bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("clip", [None, "below", "above"])
@pytest.mark.parametrize("prescale", [1.0, 0.25])
def test_adamw_restatement_matches_torch_optim(clip, prescale):
    n, steps = 1027, 7
    f32 = lambda s: float(torch.tensor(s, dtype=torch.float32))
    lr, b1, b2, eps, wd = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8), f32(1e-2)
    g = _g(11)
    p0 = torch.randn(n, generator=g).double()
    grads = [torch.randn(n, generator=g).double() * 0.1 for _ in range(steps)]
    norm = math.sqrt(R.grad_sqnorm(grads[0])) * prescale
    max_norm = {None: None, "below": f32(norm * 4), "above": f32(norm / 4)}[clip]
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(1, steps + 1):
        pt.grad = grads[t - 1] * f32(prescale)
        if clip is not None:
            torch.nn.utils.clip_grad_norm_([pt], max_norm)
        opt.step()
        ss = R.grad_sqnorm(grads[t - 1]) if clip is not None else None
        p, m, v = R.adamw_step(p, grads[t - 1], m, v, lr, b1, b2, eps, wd, t, ss, max_norm if clip is not None else 1.0, prescale)
        st = opt.state[pt]
        _close(p, pt.detach(), 1e-13)
        _close(m, st["exp_avg"], 1e-13)
        _close(v, st["exp_avg_sq"], 1e-13)


def test_stable_topk_takes_the_lowest_index_among_equals():
    x = torch.tensor([[1.0, 3.0, 3.0, -math.inf, 3.0, 2.0], [-math.inf, -math.inf, 0.5, -math.inf, -math.inf, -math.inf]])
    vals, idx, lse = R.stable_topk(x, 4)
    assert idx.tolist() == [[1, 2, 4, 5], [2, 0, 1, 3]]
    assert vals[0].tolist() == [3.0, 3.0, 3.0, 2.0] and vals[1, 0] == 0.5 and bool(torch.isinf(vals[1, 1:]).all())
    assert abs(float(lse[0]) - math.log(math.e + 3 * math.e ** 3 + math.e ** 2)) < 1e-14 and float(lse[1]) == 0.5
    assert R.argmax_rows(x).tolist() == [1, 2]
    assert R.argmax_rows(torch.full((1, 7), -math.inf)).tolist() == [0]


def test_embedding_restatements_match_autograd():
    g = _g(5)
    B, n, d, V = 3, 7, 8, 11
    tokens = torch.randint(0, V, (B, n), generator=g)
    tokens[0, 0], tokens[1, 1] = -3, V + 2
    emb, pos = torch.randn(V, d, generator=g).double().requires_grad_(True), torch.randn(n + 2, d, generator=g).double().requires_grad_(True)
    dx = torch.randn(B, n, d, generator=g).double()
    x = R.embed_tokens(tokens, emb, pos)
    assert torch.equal(x[0, 0], emb[0] + pos[0]) and torch.equal(x[1, 1], emb[V - 1] + pos[1])
    x.backward(dx)
    dtok, dpos = R.embed_tokens_bwd(dx, tokens, V)
    _close(dtok, emb.grad, 1e-15)
    _close(dpos, pos.grad[:n], 1e-15)
    sabs, cnt = R.embed_tokens_bwd_abs(dx, tokens, V)
    assert int(cnt.sum()) == B * n and bool((sabs >= dtok.abs() - 1e-12).all())


def test_attention_statistics_restatement():
    g = _g(9)
    B, Tq, Tk, H = 2, 5, 5, 2
    q, k = torch.randn(B * Tq, H * 64, generator=g).double() * 0.3, torch.randn(B * Tk, H * 64, generator=g).double()
    o, do = torch.randn(B * Tq, H * 64, generator=g).double(), torch.randn(B * Tq, H * 64, generator=g).double()
    lse, dvec = R.attention_bwd_stats(q, k, o, do, B, Tq, Tk, H, True)
    for b, h, i in ((0, 0, 0), (1, 1, 3), (1, 0, 4)):
        s = k[b * Tk: b * Tk + i + 1, 64 * h: 64 * h + 64] @ q[b * Tq + i, 64 * h: 64 * h + 64]
        assert abs(float(lse[b, h, i]) - float(torch.logsumexp(s, 0))) < 1e-13
        assert abs(float(dvec[b, h, i]) - float((o[b * Tq + i, 64 * h: 64 * h + 64] * do[b * Tq + i, 64 * h: 64 * h + 64]).sum())) < 1e-13


def test_transpose_pad_restatement():
    x = torch.arange(2 * 3 * 5, dtype=torch.float64).reshape(2, 3, 5)
    out = R.transpose_pad(x, 8, 4)
    assert out.shape == (2, 8, 4) and torch.equal(out[:, :5, :3], x.transpose(1, 2)) and float(out.abs().sum()) == float(x.abs().sum())


def test_row_kernel_entries_reject_bad_arguments_on_the_host():
    """Each call must come back LA_EINVAL from the host check, before any launch (the pointers are stand-ins)."""
    from lyricalignment_amd import _lib
    L = _lib.lib()
    P = 4096                                                          # non-null, 16-byte aligned, never dereferenced
    E = _lib.LA_EINVAL
    assert L.la_topk_rows_f32(P, 100, 4, 5, 6, P, P, P, 0) == E                                   # k > cols
    assert "topk_rows" in _lib.last_error()
    assert L.la_topk_rows_f32(P, 100, 4, 100, 0, P, P, P, 0) == E                                 # k = 0
    assert L.la_layernorm_bwd_sums_f32(P, P, P, 0, 8, 320, P, P, P, 0, 0) == E                    # d = 320 takes the scratch path
    assert "scratch" in _lib.last_error()
    assert L.la_grad_sqnorm_f32(P + 4, 8, P, 0) == E                                              # not 16-byte aligned
    assert "grad_sqnorm" in _lib.last_error()
    assert L.la_cast_f32_to_bf16(P, P + 2, 8, 0) == E                                             # y not 8-byte aligned
    assert "aligned" in _lib.last_error()
    assert L.la_embed_tokens(P, 1, 1, P, 4, P, 6, P, 0) == E                                      # d % 4 != 0
    assert "embed_tokens" in _lib.last_error()
    assert L.la_transpose_pad_f32(P, 8, 8, 4, P, 8, 4, 4, 0) == E                                 # out_cols < rows
    assert "transpose_pad" in _lib.last_error()
    assert L.la_softmax_rows_f32(P, 16, 4, 16, -1, 0) == E                                        # causal_q_len < 0
    assert "softmax_rows" in _lib.last_error()
    assert L.la_adamw_step_f32(P, P, P, P, 8, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0, 0, 1.0, 1.0, 0) == E      # step = 0
    assert "adamw_step" in _lib.last_error()
