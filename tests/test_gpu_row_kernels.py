"""The small row kernels of the training and decoding paths (csrc/la_train_elem.hip, la_optim.hip, la_resample.hip and the decoding and cast
parts of la_elementwise.hip) against the float64 restatements of tests/row_kernel_reference.py, through the C ABI, at the shapes where
each of their branches is reached: the second trip of the grid-stride loops, every LayerNorm-backward register width and rows-per-wave
choice, workgroups with absent rows, causal softmax with cols != q_len, ties / -inf / short rows in arg-max and top-k, pitched operands.

Every output is a view into a larger allocation filled with a sentinel (64 elements of slack on both sides and in the pitch columns);
the sentinel must survive the call.  Results that take one rounding per element or none are required bit for bit; the rest is
measured: error = max |a - ref| / max(|ref|, 1) against the float64 restatement must be <= 8 x E32, E32 being the error of the same
restatement evaluated by torch on the CPU in float32 on the same inputs (the factor covers the device's few-ulp expf / log1pf / tanhf
chained two deep and a 64-lane strided summation order).  Each comparison prints `kernel case err E32 ratio`; the lines of one MI355X run
are kept in profiles/row_kernel_errors.txt.  No kernel needed a term beyond 8 x E32 (GELU and GELU' with erf_fast stay below 2.2).
"""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import row_kernel_reference as R
from row_kernel_reference import RESAMPLE_CASES, resample_input

pytestmark = pytest.mark.gpu

SLACK = 64
FACTOR = 8.0
NULL = 0


def _L():
    from lyricalignment_amd import _lib
    _lib.require_gpu()
    return _lib.lib()


def _ok(rc, what):
    from lyricalignment_amd import _lib
    _lib.check(rc, what)


def _st():
    from lyricalignment_amd import _lib
    return _lib.stream_ptr()


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _dev(t):
    return t.contiguous().cuda()


def _contig(shape):
    st, acc = [], 1
    for s in reversed(shape):
        st.append(acc)
        acc *= s
    return tuple(reversed(st))


class Guard:
    """An output of `shape` (element strides `strides`, contiguous by default) inside a sentinel-filled allocation."""

    def __init__(self, shape, strides=None, dtype=torch.float32):
        self.shape = tuple(shape)
        self.strides = tuple(strides) if strides is not None else _contig(self.shape)
        span = 1 + sum((s - 1) * st for s, st in zip(self.shape, self.strides))
        self.sent = 7.0 if dtype.is_floating_point else 0x7F7F
        self.buf = torch.full((SLACK + span + SLACK,), self.sent, dtype=dtype, device="cuda")
        self.view = self.buf.as_strided(self.shape, self.strides, SLACK)

    @property
    def ptr(self):
        return self.buf.data_ptr() + SLACK * self.buf.element_size()

    def set(self, t):
        self.view.copy_(t.to(self.buf.dtype))
        return self

    def get(self):
        torch.cuda.synchronize()
        return self.view.cpu().contiguous()

    def check(self, untouched=False):
        """Every sentinel outside the view is intact (untouched=True: inside it as well)."""
        torch.cuda.synchronize()
        host = self.buf.cpu()
        keep = torch.ones(host.numel(), dtype=torch.bool)
        if not untouched:
            keep.as_strided(self.shape, self.strides, SLACK).fill_(False)
        assert bool((host[keep] == self.sent).all()), "a guard element was overwritten"


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def _same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    assert torch.equal(_bits(got), _bits(want)), f"{int((_bits(got) != _bits(want)).sum())} elements differ"


def _measured(kernel, case, got, ref, e32_value):
    """err <= 8 E32; prints the figures first."""
    err, e32 = R.rel_err(got, ref), R.rel_err(e32_value, ref)
    ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else math.inf)
    print(f"{kernel} {case} {err:.3e} {e32:.3e} {ratio:.2f}")
    assert err <= FACTOR * e32, (kernel, case, err, e32)


# ---- elementwise: second trip of the grid-stride loop -------------------------------------------------------------------------------

EW_SIZES = [1, 255, 257, 1048576 + 257]
_POINTS = torch.tensor([-100.0, -88.0, -20.0, 0.0, 19.999, 20.0, 20.001, 88.0])
_GRID = torch.linspace(-30.0, 30.0, 241)


def _ew_values(n, seed):
    """N(0, 3^2), the branch points and a grid over [-30, 30]: after element 0 and, for long inputs, again at the very end (the region only
    the second trip of the loop reaches)."""
    x = torch.randn(n, generator=_g(seed)) * 3
    fixed = torch.cat([_POINTS, _GRID])
    m = min(n - 1, fixed.numel())
    if m > 0:
        x[1:1 + m] = fixed[:m]
    if n > 4 * fixed.numel():
        x[n - fixed.numel():] = fixed
    return x


def _ew_mask(n, seed):
    m = (torch.rand(n, generator=_g(seed)) < 0.5).to(torch.uint8)
    m[0::256] = 1
    m[1::256] = 0
    return m


@pytest.mark.parametrize("n", EW_SIZES)
def test_elementwise_activations(n):
    L = _L()
    x, dy = _ew_values(n, n), torch.randn(n, generator=_g(n + 1))
    xd, dyd = _dev(x), _dev(dy)
    x64, dy64 = x.double(), dy.double()
    for name, fwd in (("la_mish_f32", R.mish), ("la_gelu_f32", R.gelu)):
        y = Guard((n,))
        _ok(getattr(L, name)(xd.data_ptr(), y.ptr, n, _st()), name)
        y.check()
        _measured(name, f"n={n}", y.get(), fwd(x64), fwd(x))
    for name, bwd in (("la_mish_bwd_f32", R.mish_bwd), ("la_gelu_bwd_f32", R.gelu_bwd)):
        dx = Guard((n,))
        _ok(getattr(L, name)(xd.data_ptr(), dyd.data_ptr(), dx.ptr, n, _st()), name)
        dx.check()
        _measured(name, f"n={n}", dx.get(), bwd(x64, dy64), bwd(x, dy))


@pytest.mark.parametrize("n", EW_SIZES)
def test_elementwise_add_scale_mask_are_exact(n):
    L = _L()
    a, b, mask = _ew_values(n, n + 2), torch.randn(n, generator=_g(n + 3)), _ew_mask(n, n + 4)
    ad, bd, md = _dev(a), _dev(b), _dev(mask)
    alpha = torch.tensor(1 / 0.9, dtype=torch.float32)
    y = Guard((n,))
    _ok(L.la_add_f32(ad.data_ptr(), bd.data_ptr(), y.ptr, n, _st()), "add")
    y.check()
    _same_bits(y.get(), a + b)
    y = Guard((n,))
    _ok(L.la_scale_f32(ad.data_ptr(), float(alpha), y.ptr, n, _st()), "scale")
    y.check()
    _same_bits(y.get(), a * alpha)
    y = Guard((n,))
    _ok(L.la_mask_scale_f32(ad.data_ptr(), md.data_ptr(), float(alpha), y.ptr, n, _st()), "mask_scale")
    y.check()
    _same_bits(y.get(), torch.where(mask != 0, a * alpha, torch.zeros(n)))
    if n > 256:
        assert 0 < int(mask[-256:].sum()) < 256


# ---- optimizer ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 5, 1027, 4195333])
def test_grad_sqnorm_adds_into_the_accumulator(n):
    """Squares are exact in double and the n additions happen in some order: relative error <= n 2^-52 against the float64 sum."""
    L = _L()
    g1, g2 = torch.randn(n, generator=_g(n)) * 0.3, torch.randn(n, generator=_g(n + 1)) * 2
    s1, s2 = R.grad_sqnorm(g1), R.grad_sqnorm(g2)
    g1d, g2d = _dev(g1), _dev(g2)
    for preset in (0.0, 3.5):
        acc = Guard((1,), dtype=torch.float64).set(torch.tensor([preset], dtype=torch.float64))
        _ok(L.la_grad_sqnorm_f32(g1d.data_ptr(), n, acc.ptr, _st()), "grad_sqnorm")
        one = float(acc.get()[0])
        _ok(L.la_grad_sqnorm_f32(g2d.data_ptr(), n, acc.ptr, _st()), "grad_sqnorm")       # a second bucket into the same accumulator
        two = float(acc.get()[0])
        acc.check()
        for got, want, terms in ((one, preset + s1, n + 1), (two, preset + s1 + s2, 2 * n + 2)):
            err, bound = abs(got - want) / want, terms * 2.0 ** -52
            print(f"la_grad_sqnorm_f32 n={n},preset={preset},terms={terms} {err:.3e} bound={bound:.3e}")
            assert err <= bound


@pytest.mark.parametrize("n", [5, 2097155])
def test_adamw_step(n):
    L = _L()
    f32 = lambda s: float(torch.tensor(s, dtype=torch.float32))
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 1e-2
    g = _g(n)
    p0, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    m0, v0 = torch.randn(n, generator=g) * 0.05, torch.rand(n, generator=g) * 0.01
    grd = _dev(gr)
    sum_sq = R.grad_sqnorm(gr)
    ssd = torch.tensor([sum_sq], dtype=torch.float64).cuda()
    for step in (1, 7):
        for prescale in (1.0, 0.25):
            norm = math.sqrt(sum_sq) * prescale
            for clip, max_norm in ((None, 1.0), ("below", f32(norm * 4)), ("above", f32(norm / 4))):
                p, m, v = Guard((n,)).set(p0), Guard((n,)).set(m0), Guard((n,)).set(v0)
                _ok(L.la_adamw_step_f32(p.ptr, grd.data_ptr(), m.ptr, v.ptr, n, lr, b1, b2, eps, wd, step,
                                        ssd.data_ptr() if clip else NULL, max_norm, prescale, _st()), "adamw_step")
                ss = sum_sq if clip else None
                ref = R.adamw_step(p0.double(), gr.double(), m0.double(), v0.double(), lr, b1, b2, eps, wd, step, ss, max_norm, prescale)
                e32 = R.adamw_step(p0, gr, m0, v0, lr, b1, b2, eps, wd, step, ss, max_norm, prescale)
                case = f"n={n},step={step},prescale={prescale},clip={clip}"
                for out, name, r, e in zip((p, m, v), "pmv", ref, e32):
                    out.check()
                    _measured("la_adamw_step_f32", f"{case},{name}", out.get(), r, e)
                if clip == "above":              # the clip took effect: m differs from the unclipped one
                    assert R.rel_err(ref[1], R.adamw_step(p0.double(), gr.double(), m0.double(), v0.double(), lr, b1, b2, eps, wd, step,
                                                          None, 1.0, prescale)[1]) > 1e-4


# ---- casts --------------------------------------------------------------------------------------------------------------------------

_F32_MAX = 3.4028234663852886e38
_CAST_SPECIALS = torch.tensor([1.00390625, 1.01171875, 0.0, -0.0, math.inf, -math.inf, _F32_MAX, -_F32_MAX, math.nan, 1.0, -1.00390625],
                              dtype=torch.float32)


@pytest.mark.parametrize("n", [1, 3, 4, 7, 4195333])
def test_cast_f32_to_bf16_rounds_to_nearest_even(n):
    L = _L()
    x = torch.randn(n, generator=_g(n)) * torch.exp(torch.randn(n, generator=_g(n + 1)) * 8)
    k = min(n, _CAST_SPECIALS.numel())
    x[:k] = _CAST_SPECIALS[:k]                          # ties first: 1.00390625 -> 1.0, 1.01171875 -> 1.015625
    if n > 64:
        x[n - _CAST_SPECIALS.numel():] = _CAST_SPECIALS.flip(0)      # the scalar tail (n % 4 elements) rounds a tie too
    y, xd = Guard((n,), dtype=torch.int16), _dev(x)
    _ok(L.la_cast_f32_to_bf16(xd.data_ptr(), y.ptr, n, _st()), "cast_f32_to_bf16")
    y.check()
    got, want = y.get().view(torch.bfloat16), x.to(torch.bfloat16)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    _same_bits(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want))
    assert float(got[0]) == 1.0 and (n < 2 or float(got[1]) == 1.015625)
    if n > 64:
        assert float(got[-1]) == 1.0 and bool(torch.isinf(got[6])) and bool(torch.isnan(got[8]))


@pytest.mark.parametrize("n", [1, 77, 1048653])
def test_cast_bf16_to_f32_is_exact(n):
    L = _L()
    bits = torch.randint(-32768, 32768, (n,), generator=_g(n), dtype=torch.int32).to(torch.int16)      # every pattern, NaN payloads included
    y, bd = Guard((n,)), _dev(bits)
    _ok(L.la_cast_bf16_to_f32(bd.data_ptr(), y.ptr, n, _st()), "cast_bf16_to_f32")
    y.check()
    assert torch.equal(_bits(y.get()), (bits.to(torch.int32) & 0xFFFF) << 16)


# ---- layout -------------------------------------------------------------------------------------------------------------------------

TP_CASES = [(1, 1, 1, 1), (31, 33, 64, 32), (33, 31, 31, 33), (64, 64, 64, 64), (70, 5, 8, 96)]


@pytest.mark.parametrize("rows,cols,out_rows,out_cols", TP_CASES)
def test_transpose_pad_plain_and_batched(rows, cols, out_rows, out_cols):
    L = _L()
    ld_in, ld_out, batch = cols + 3, out_cols + 5, 3
    bs_in, bs_out = rows * ld_in + 7, out_rows * ld_out + 11
    src = torch.randn(batch * bs_in, generator=_g(rows * cols))
    xin = src.as_strided((batch, rows, cols), (bs_in, ld_in, 1))
    want = R.transpose_pad(xin, out_rows, out_cols)
    sd = _dev(src)
    out = Guard((out_rows, out_cols), (ld_out, 1))
    _ok(L.la_transpose_pad_f32(sd.data_ptr(), ld_in, rows, cols, out.ptr, ld_out, out_rows, out_cols, _st()), "transpose_pad")
    out.check()
    _same_bits(out.get(), want[0])
    out = Guard((batch, out_rows, out_cols), (bs_out, ld_out, 1))
    _ok(L.la_transpose_pad_batched_f32(sd.data_ptr(), ld_in, bs_in, rows, cols, out.ptr, ld_out, bs_out, out_rows, out_cols, batch, _st()),
        "transpose_pad_batched")
    out.check()
    _same_bits(out.get(), want)


@pytest.mark.parametrize("B,T,stride,C,rows_out", [(1, 1, 1, 1, 3), (2, 5, 1, 3, 7), (2, 5, 2, 3, 11), (1, 4, 2, 8, 12), (3, 750, 2, 5, 1502)])
def test_col2im3_overlap_add(B, T, stride, C, rows_out):
    L = _L()
    dcols = torch.randn(B, T, 3, C, generator=_g(T + C))
    out, dd = Guard((B, rows_out, C)), _dev(dcols)
    _ok(L.la_col2im3_f32(dd.data_ptr(), B, T, stride, C, out.ptr, rows_out, _st()), "col2im3")
    out.check()
    _same_bits(out.get(), R.col2im3(dcols, stride, rows_out))
    assert R.rel_err(out.get(), R.col2im3(dcols.double(), stride, rows_out)) <= 3 * 2.0 ** -24


# ---- token embedding ----------------------------------------------------------------------------------------------------------------

def _tokens(B, n, V, seed):
    t = torch.randint(0, V, (B, n), generator=_g(seed))
    if n >= 5:
        t[:, 1] = t[:, 0]                    # every clip repeats a token
        t[:, 2] = V // 2                     # one token shared by all clips
        t[0, 3], t[B - 1, 4] = -3, V + 2     # clamped to 0 and V - 1
    else:
        t[0, 0] = -3
    return t


@pytest.mark.parametrize("B,n,d,V", [(1, 1, 4, 2), (3, 7, 64, 11), (4, 33, 1028, 50)])
def test_embed_tokens_forward_and_backward(B, n, d, V):
    L = _L()
    g = _g(B * n + d)
    tok = _tokens(B, n, V, d)
    emb, pos, dx = torch.randn(V, d, generator=g), torch.randn(n + 1, d, generator=g), torch.randn(B, n, d, generator=g)
    tokd, embd, posd = _dev(tok), _dev(emb), _dev(pos)
    x = Guard((B * n, d))
    _ok(L.la_embed_tokens(tokd.data_ptr(), B, n, embd.data_ptr(), V, posd.data_ptr(), d, x.ptr, _st()), "embed_tokens")
    x.check()
    _same_bits(x.get().reshape(B, n, d), R.embed_tokens(tok, emb, pos))
    dxd = _dev(dx)
    sabs, cnt = R.embed_tokens_bwd_abs(dx, tok, V)
    ref_tok, _ = R.embed_tokens_bwd(dx.double(), tok, V)
    _, want_pos = R.embed_tokens_bwd(dx, tok, V)
    for preset in (None, torch.randn(V, d, generator=g)):
        dtok = Guard((V, d)).set(torch.zeros(V, d) if preset is None else preset)
        dpos = Guard((n, d))
        _ok(L.la_embed_tokens_bwd_f32(dxd.data_ptr(), tokd.data_ptr(), B, n, d, V, dtok.ptr, dpos.ptr, _st()), "embed_tokens_bwd")
        dtok.check()
        dpos.check()
        _same_bits(dpos.get(), want_pos)
        # float atomics in any order: |error| <= c 2^-23 sum |g| over the c contributions of the element (a preset value is one of them)
        ref, s, c = ref_tok, sabs, cnt
        if preset is not None:
            ref, s, c = ref_tok + preset.double(), sabs + preset.double().abs(), cnt + 1
        err = (dtok.get().double() - ref).abs()
        print(f"la_embed_tokens_bwd_f32 B={B},n={n},d={d},V={V},preset={preset is not None} dtok {float(err.max()):.3e} "
              f"bound={float((c * 2.0 ** -23 * s).max()):.3e}")
        assert bool((err <= c * 2.0 ** -23 * s).all())
        assert bool((dtok.get()[cnt[:, 0] == 0] == (0 if preset is None else preset[cnt[:, 0] == 0])).all())      # untouched rows keep their value


# ---- softmax rows -------------------------------------------------------------------------------------------------------------------

def _softmax_case(rows, cols, ld, q_len, tag):
    L = _L()
    g = _g(rows * 1000 + cols + ld)
    s = torch.randn(rows, cols, generator=g) * 4
    s[0, cols // 2] += 80.0                                  # one row with a spike
    pad = torch.randn(rows, ld, generator=g)
    pad[:, :cols] = s
    buf = Guard((rows, ld)).set(pad)                         # the kernel owns all ld columns of a row: pad columns become 0
    _ok(L.la_softmax_rows_f32(buf.ptr, ld, rows, cols, q_len, _st()), "softmax_rows")
    buf.check()
    got = buf.get()
    vis = R.causal_visible(rows, cols, q_len)
    assert bool((got[:, cols:] == 0).all()) and bool((got[:, :cols][~vis] == 0).all())
    ref, e32 = R.softmax_rows(s.double(), q_len), R.softmax_rows(s, q_len)
    case = f"rows={rows},cols={cols},ld={ld},{tag}"
    _measured("la_softmax_rows_f32", case, got[:, :cols], ref, e32)
    _measured("la_softmax_rows_f32", case + ",rowsum", got[:, :cols].double().sum(1), torch.ones(rows, dtype=torch.float64), e32.double().sum(1))
    # backward on the float32 probabilities the restatement gives (masked entries are exact zeros there as well)
    dp = torch.randn(rows, ld, generator=g)
    p32 = torch.zeros(rows, ld)
    p32[:, :cols] = e32
    dbuf, pd = Guard((rows, ld)).set(dp), _dev(p32)
    _ok(L.la_softmax_bwd_rows_f32(pd.data_ptr(), dbuf.ptr, ld, rows, cols, _st()), "softmax_bwd_rows")
    dbuf.check()
    dgot = dbuf.get()
    assert bool((dgot[:, cols:] == 0).all()) and bool((dgot[:, :cols][~vis] == 0).all())
    _measured("la_softmax_bwd_rows_f32", case, dgot[:, :cols], R.softmax_bwd_rows(e32.double(), dp[:, :cols].double()),
              R.softmax_bwd_rows(e32, dp[:, :cols]))


@pytest.mark.parametrize("cols", [1, 63, 64, 65, 333])
def test_softmax_rows_forward_and_backward(cols):
    for rows in (1, 3, 6):                                   # workgroups of 4 rows with absent rows
        for ld in (cols, cols + 5):
            _softmax_case(rows, cols, ld, 0, "plain")


@pytest.mark.parametrize("q_len,cols", [(5, 5), (37, 37), (3, 10), (1, 9), (6, 3)])
def test_softmax_rows_causal(q_len, cols):
    """Row r is query r mod q_len and sees keys 0 .. (r mod q_len) + cols - q_len; with cols < q_len ((6, 3)) the queries that would see
    no key see key 0, as include/lyricalign.h states."""
    for ld in (cols, cols + 5):
        _softmax_case(2 * q_len, cols, ld, q_len, f"causal_q_len={q_len}")


# ---- LayerNorm backward -------------------------------------------------------------------------------------------------------------

def _ln_inputs(M, d):
    g = _g(M + d)
    x = torch.randn(M, d, generator=g) * torch.exp(torch.randn(M, 1, generator=g))
    return x, torch.randn(M, d, generator=g), torch.randn(M, d, generator=g), torch.rand(d, generator=g) + 0.5


def _ln_case(M, d, offset=0):
    """Both entries, with and without `residual`, on one set of inputs (one float64 and one float32 evaluation of the restatement).
    offset: x starts `offset` floats past a 16-byte boundary (the register form is refused, the scratch form runs)."""
    L = _L()
    x, dy, res, gamma = _ln_inputs(M, d)
    xbuf = torch.zeros(M * d + 4, device="cuda")
    xbuf[offset:offset + M * d] = x.reshape(-1).cuda()
    x_ptr = xbuf.data_ptr() + 4 * offset
    dyd, resd, gd = _dev(dy), _dev(res), _dev(gamma)
    fast = d % 256 == 0 and d <= 2048 and offset == 0
    ref = R.layernorm_bwd(x.double(), dy.double(), gamma.double())
    e32 = R.layernorm_bwd(x, dy, gamma)
    for with_residual in (True, False):
        case = f"M={M},d={d},residual={int(with_residual)},offset={offset}"
        dx, dg, db = Guard((M, d)), Guard((d,)), Guard((d,))
        scratch = None if fast else Guard((M, d))
        _ok(L.la_layernorm_bwd_sums_f32(x_ptr, dyd.data_ptr(), gd.data_ptr(), resd.data_ptr() if with_residual else NULL, M, d, dx.ptr, dg.ptr,
                                        db.ptr, scratch.ptr if scratch else NULL, _st()), "layernorm_bwd_sums")
        want_dx, e32_dx = (res.double() + ref[0], res + e32[0]) if with_residual else (ref[0], e32[0])
        for out, name, r, e in ((dx, "dx", want_dx, e32_dx), (dg, "dgamma", ref[2], e32[2]), (db, "dbeta", ref[3], e32[3])):
            out.check()
            _measured("la_layernorm_bwd_sums_f32", f"{case},{name}", out.get(), r, e)
        if scratch:
            scratch.check()
    dx, dyx = Guard((M, d)), Guard((M, d))
    _ok(L.la_layernorm_bwd_f32(x_ptr, dyd.data_ptr(), gd.data_ptr(), M, d, dx.ptr, dyx.ptr, _st()), "layernorm_bwd")
    for out, name, i in ((dx, "dx", 0), (dyx, "dy_xhat", 1)):
        out.check()
        _measured("la_layernorm_bwd_f32", f"M={M},d={d},offset={offset},{name}", out.get(), ref[i], e32[i])


@pytest.mark.parametrize("nv", [1, 2, 3, 4, 5, 6, 7, 8])
def test_layernorm_backward_every_register_width(nv):
    _ln_case(517, 256 * nv)


@pytest.mark.parametrize("M", [1, 3, 5, 9001, 20003, 40001, 65411])
def test_layernorm_backward_every_rows_per_wave_choice(M):
    """d = 256: 2, 2, 2, 4, 8, 16, 32 rows per wave, a ragged last wave each time (and waves whose first row is past M)."""
    _ln_case(M, 256)


@pytest.mark.parametrize("d,offset", [(4, 0), (320, 0), (2304, 0), (256, 1)])
def test_layernorm_backward_scratch_form(d, offset):
    _ln_case(37, d, offset)


# ---- cross entropy ------------------------------------------------------------------------------------------------------------------

def _ce_inputs(rows, V):
    """Rows 0 and 1 carry the +1e4 and -1e4 offsets and always count; the ignored targets (-100, -5, >= V) sit on other rows."""
    g = _g(rows * 7 + V)
    logits = torch.randn(rows, V, generator=g) * 3
    target = torch.randint(0, V, (rows,), generator=g)
    if rows >= 3:
        logits[0] += 1e4
        logits[1] -= 1e4
    if rows == 3:
        target[2] = -5 if V % 2 == 0 else V          # ignored like -100
    if rows >= 4:
        target[2], target[3] = -100, V + 1
    if rows >= 5:
        target[4] = -5
    return logits, target


def _ce_case(rows, V, ld, logits, target, with_grad, tag):
    L = _L()
    ld_d, scale = V + 1, 0.125
    lbuf = torch.randn(rows, ld, generator=_g(3))
    lbuf[:, :V] = logits
    loss2, ws = Guard((2,)), Guard((2 * rows,))
    dl = Guard((rows, V), (ld_d, 1)) if with_grad else None
    ld_, td = _dev(lbuf), _dev(target)
    _ok(L.la_cross_entropy_f32(ld_.data_ptr(), ld, rows, V, td.data_ptr(), scale, loss2.ptr, ws.ptr,
                               dl.ptr if dl else NULL, ld_d, _st()), "cross_entropy")
    loss2.check()
    ws.check()
    got = loss2.get()
    ref, e32 = R.cross_entropy(logits.double(), target, scale), R.cross_entropy(logits, target, scale)
    case = f"rows={rows},V={V},ld={ld},{tag}"
    count = int(((target >= 0) & (target < V)).sum())
    if count == 0:
        assert math.isnan(float(got[0])) and float(got[1]) == 0.0
    else:
        assert float(got[1]) == float(np.float32(1.0) / np.float32(count))
        _measured("la_cross_entropy_f32", case + ",loss", got[:1], ref[0].reshape(1), e32[0].reshape(1))
    if dl:
        dl.check()
        if count == 0:
            assert bool((dl.get() == 0).all())
        else:
            _measured("la_cross_entropy_f32", case + ",dlogits", dl.get(), ref[2], e32[2])
            assert bool((dl.get()[(target < 0) | (target >= V)] == 0).all())


@pytest.mark.parametrize("rows,V", [(1, 1), (4, 5), (3, 256), (3, 257), (64, 51865)])
def test_cross_entropy(rows, V):
    logits, target = _ce_inputs(rows, V)
    for ld in (V, V + 3):
        _ce_case(rows, V, ld, logits, target, True, "grad")
    _ce_case(rows, V, V + 3, logits, target, False, "no_grad")
    _ce_case(rows, V, V, logits, torch.where(torch.arange(rows) % 2 == 0, torch.full((rows,), -100), torch.full((rows,), V + 7)), True, "all_ignored")


# ---- arg-max and top-k --------------------------------------------------------------------------------------------------------------

def _argmax_rows(cols):
    g = _g(cols)
    rows = [torch.randn(cols, generator=g)]
    rows.append(torch.full((cols,), 1.5))                                   # all equal: 0
    r = torch.full((cols,), -math.inf)
    r[cols // 3] = -2.0
    rows.append(r)                                                          # -inf except one entry
    rows.append(torch.full((cols,), -math.inf))                             # all -inf: 0
    r = torch.randn(cols, generator=g)
    r[cols - 1] = 9.0
    rows.append(r)                                                          # the maximum in the last column
    pairs = [(1, 3)] if cols >= 5 else []
    if cols >= 255:
        pairs.append((3, 70))                                               # two waves of the workgroup
        pairs.append((200, 63))                                             # the later index first in its wave's butterfly
    if cols >= 257:
        pairs.append((0, 256))                                              # one lane's stride
    if cols >= 3001:
        pairs += [(10, 266), (2999, 2743), (300, 3000)]
    for a, b in pairs:
        r = torch.randn(cols, generator=g)
        r[a] = r[b] = 8.0
        rows.append(r)
    return torch.stack(rows)


@pytest.mark.parametrize("cols", [1, 5, 255, 256, 257, 3001])
def test_argmax_rows_takes_the_first_maximum(cols):
    L = _L()
    x = _argmax_rows(cols)
    rows, ld = x.shape[0], cols + 3
    xp = torch.full((rows, ld), 100.0)                   # pitch columns hold values above every entry: they must not be read
    xp[:, :cols] = x
    out, xd = Guard((rows,), dtype=torch.int64), _dev(xp)
    _ok(L.la_argmax_rows_f32(xd.data_ptr(), ld, rows, cols, out.ptr, _st()), "argmax_rows")
    out.check()
    want = R.argmax_rows(x)
    assert out.get().tolist() == want.tolist()
    assert want[1] == 0 and want[2] == cols // 3 and want[3] == 0 and want[4] == cols - 1


def _topk_rows(cols, k):
    g = _g(cols * 10 + k)
    rows = [torch.randn(cols, generator=g) * 3]
    if cols >= 3:
        r = torch.randn(cols, generator=g)
        for c in sorted({cols - 1, cols // 2, 1}):
            r[c] = 7.0
        rows.append(r)                                                      # three equal maxima, taken in index order
        r = torch.randn(cols, generator=g)
        r[torch.randperm(cols, generator=g)[: cols // 2]] = -math.inf
        rows.append(r)                                                      # -inf in half the columns
        rows.append(torch.full((cols,), 0.25))                              # all equal: indices 0 .. k-1
    if k >= 2:
        r = torch.full((cols,), -math.inf)
        r[torch.randperm(cols, generator=g)[: k - 1]] = torch.randn(k - 1, generator=g)
        rows.append(r)                                                      # k - 1 finite entries: the last pick is a -inf at the lowest free index
    return torch.stack(rows)


@pytest.mark.parametrize("cols,k", [(1, 1), (5, 5), (8, 8), (200, 8), (257, 3), (51865, 8)])
def test_topk_rows_values_indices_and_lse(cols, k):
    L = _L()
    x = _topk_rows(cols, k)
    rows, ld = x.shape[0], cols + 3
    xp = torch.full((rows, ld), 100.0)
    xp[:, :cols] = x
    vals, idx, lse, xd = Guard((rows, k)), Guard((rows, k), dtype=torch.int64), Guard((rows,)), _dev(xp)
    _ok(L.la_topk_rows_f32(xd.data_ptr(), ld, rows, cols, k, vals.ptr, idx.ptr, lse.ptr, _st()), "topk_rows")
    for o in (vals, idx, lse):
        o.check()
    wv, wi, wl = R.stable_topk(x, k)
    assert idx.get().tolist() == wi.tolist()
    assert torch.equal(vals.get(), wv)
    assert bool(torch.isfinite(wl).all()) and bool(torch.isfinite(lse.get()).all())
    _measured("la_topk_rows_f32", f"cols={cols},k={k},lse", lse.get(), wl, torch.logsumexp(x, 1))
    if k >= 2:
        assert math.isinf(float(vals.get()[-1, k - 1])) and int(idx.get()[-1, k - 1]) == int(torch.isinf(x[-1]).nonzero()[0])


# ---- attention backward statistics --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,Tq,Tk,H,causal", [(1, 1, 1, 1, False), (2, 37, 37, 2, True), (1, 70, 200, 1, False), (2, 65, 129, 2, False)])
def test_attention_backward_statistics(B, Tq, Tk, H, causal):
    L = _L()
    g = _g(Tq * 3 + Tk)
    d = 64 * H
    q, k = torch.randn(B * Tq, d, generator=g) * 0.35, torch.randn(B * Tk, d, generator=g)
    o, do = torch.randn(B * Tq, d, generator=g), torch.randn(B * Tq, d, generator=g)
    ld = d + 4                                           # pitched operands, rows still 16-byte aligned

    def pitched(t):
        p = torch.full((t.shape[0], ld), 50.0)
        p[:, :d] = t
        return _dev(p)

    qd, kd, od, dod = pitched(q), pitched(k), pitched(o), pitched(do)
    ref = R.attention_bwd_stats(q.double(), k.double(), o.double(), do.double(), B, Tq, Tk, H, causal)
    e32 = R.attention_bwd_stats(q, k, o, do, B, Tq, Tk, H, causal)
    case = f"B={B},Tq={Tq},Tk={Tk},H={H},causal={int(causal)}"
    lse, dvec = Guard((B, H, Tq)), Guard((B, H, Tq))
    _ok(L.la_attention_bwd_stats_f32(qd.data_ptr(), ld, kd.data_ptr(), ld, od.data_ptr(), ld, dod.data_ptr(), ld, B, Tq, Tk, H, int(causal),
                                     NULL, lse.ptr, dvec.ptr, _st()), "attention_bwd_stats")
    lse.check()
    dvec.check()
    _measured("la_attention_bwd_stats_f32", case + ",lse", lse.get(), ref[0], e32[0])
    _measured("la_attention_bwd_stats_f32", case + ",dvec", dvec.get(), ref[1], e32[1])
    # lse handed in: only dvec is written
    lse_in = _dev(e32[0])
    lse2, dvec2 = Guard((B, H, Tq)), Guard((B, H, Tq))
    _ok(L.la_attention_bwd_stats_f32(qd.data_ptr(), ld, kd.data_ptr(), ld, od.data_ptr(), ld, dod.data_ptr(), ld, B, Tq, Tk, H, int(causal),
                                     lse_in.data_ptr(), lse2.ptr, dvec2.ptr, _st()), "attention_bwd_stats")
    lse2.check(untouched=True)
    dvec2.check()
    torch.cuda.synchronize()
    assert torch.equal(lse_in.cpu(), e32[0].contiguous())
    _measured("la_attention_bwd_stats_f32", case + ",dvec,lse_in", dvec2.get(), ref[1], e32[1])


# ---- resampling ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sr,n_in", RESAMPLE_CASES)
def test_resample_to_16k_matches_scipy(sr, n_in):
    """up > down (8, 11.025, 12 kHz), inputs shorter than the filter, and the down > up ratios: scipy.signal.resample_poly on the float64
    input, atol 2e-6 as in test_audio_loader_resample_matches_scipy; the same launch into a guarded buffer gives the same bits."""
    from scipy.signal import resample_poly
    from lyricalignment_amd.utils.audio import _design, resample_to_16k
    L = _L()
    fr = Fraction(16000, sr)
    up, down = fr.numerator, fr.denominator
    x = resample_input(sr, n_in)
    want = resample_poly(x, up, down)
    got = resample_to_16k(x.astype(np.float32), sr)
    assert got.dtype == np.float32 and got.shape == want.shape
    err = float(np.abs(got - want).max())
    print(f"la_resample_poly_f32 sr={sr},n_in={n_in} {err:.3e} atol=2e-6")
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)
    h, skip = _design(up, down)
    y, xd, hd = Guard((got.shape[0],)), _dev(torch.from_numpy(x.astype(np.float32))), _dev(torch.from_numpy(h))
    _ok(L.la_resample_poly_f32(xd.data_ptr(), n_in, hd.data_ptr(), h.shape[0], up, down, skip, y.ptr, got.shape[0], _st()), "resample_poly")
    y.check()
    _same_bits(y.get(), torch.from_numpy(got))
