"""The 256 x 256 GEMM kernel's two interior-tile epilogue forms for 16-bit results without a residual (library option gemm_epi16,
include/lyricalign.h): 0 = the tile crosses the LDS transpose as float32 and the arithmetic runs on row-major quads, 1 = the arithmetic
runs in the accumulator layout and the tile crosses as 16-bit values (la_gemm_epilogue.h wave_epilogue16).  Same operands, same
operations in the same order per element: the raw 16-bit outputs must be identical.

Shapes: M = 2 * 256 + 17, N = 2 * 256 + 64 -- the smallest with interior and edge wave tiles in both directions (option gemm_tile = 512
puts them on the 256 x 256 kernel) -- at K = 256 (the hand-placed loop's minimum) and K = 192 (the quadrant ping-pong loop)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M, N = 2 * 256 + 17, 2 * 256 + 64
KS = (256, 192)
DTYPES = (torch.bfloat16, torch.float16)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.fixture
def forms():
    """forms(fn) -> (fn() with the float32 staging, fn() with the 16-bit staging), both on the 256 x 256 kernel; options restored."""
    from lyricalignment_amd import _lib
    prev = _lib.get_option("gemm_epi16")

    def run(fn):
        with _lib.option("gemm_tile", 512):
            _lib.set_option("gemm_epi16", 0)
            old = fn()
            _lib.set_option("gemm_epi16", 1)
            new = fn()
        return old, new

    yield run
    _lib.set_option("gemm_epi16", prev)


def _same_bits(old, new):
    assert old.dtype == new.dtype and old.dtype in DTYPES
    assert torch.equal(old.view(torch.int16), new.view(torch.int16))


def _one_hot_operands(K, dtype):
    """out[m][n] = a(m) W[n][k(m)] + bias[n] with small integers and eighths: exact in both 16-bit types, and a function of the element's own
    row (a(m), k(m)) and column (W row n, bias[n]) -- a quad that lands in another row or four columns aside cannot pass."""
    m = torch.arange(M)
    a = torch.zeros(M, K)
    a[m, m % K] = (1 + m % 5).float()
    n = torch.arange(N)
    w = ((n[:, None] + 3 * torch.arange(K)[None, :]) % 7 - 3).float()
    bias = (n % 61).float() * 0.125 - 3.0
    ref = (1 + m % 5).float()[:, None] * w[:, m % K].T + bias[None, :]
    return a.to(dtype).cuda(), w.to(dtype).cuda(), bias.cuda(), ref


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", KS)
def test_option_exists_and_one_hot_rows_land_in_their_own_row_and_column(K, dtype, forms):
    from lyricalignment_amd import _lib, ops
    with _lib.option("gemm_epi16", 1):
        assert _lib.get_option("gemm_epi16") == 1
    a, w, bias, ref = _one_hot_operands(K, dtype)
    old, new = forms(lambda: ops.gemm(a, w, bias=bias).clone())
    assert torch.equal(new.float().cpu(), ref)          # exact: every value is representable
    _same_bits(old, new)
    old, new = forms(lambda: ops.gemm(a, w).clone())    # no bias
    assert torch.equal(new.float().cpu(), ref - bias.cpu()[None, :])
    _same_bits(old, new)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", KS)
def test_bias_and_gelu_same_bits_and_close_to_float64(K, dtype, forms):
    """Seeded random operands: both forms against each other (bits) and against a float64 product of the rounded operands at the tolerance
    tests/test_gpu_ops.py test_gemm_epilogues holds the 16-bit results of this kernel to (rtol = atol = 1e-2)."""
    from lyricalignment_amd import ops
    a = _rand(M, K, seed=301, scale=0.3).to(dtype); w = _rand(N, K, seed=302, scale=0.3).to(dtype)
    bias = _rand(N, seed=303)
    base = a.double() @ w.double().T + bias.double()
    ad, wd, bd = a.cuda(), w.cuda(), bias.cuda()
    old, new = forms(lambda: ops.gemm(ad, wd, bias=bd).clone())
    _same_bits(old, new)
    np.testing.assert_allclose(new.double().cpu().numpy(), base.numpy(), rtol=1e-2, atol=1e-2)
    old, new = forms(lambda: ops.gemm(ad, wd, bias=bd, gelu=True).clone())
    _same_bits(old, new)
    np.testing.assert_allclose(new.double().cpu().numpy(), torch.nn.functional.gelu(base).numpy(), rtol=1e-2, atol=1e-2)
    old, new = forms(lambda: ops.gemm(ad, wd, bias=bd, gelu="erf").clone())
    _same_bits(old, new)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", KS)
def test_layernorm_consumer_statistics_reach_their_row_block(K, dtype, forms):
    """LayerNorm-consumer epilogue rstd (acc - mean c) + b with and without GELU.  Every third row has (mean, rstd) = (0, 1), the others a
    large mean and an rstd of their own: statistics handed to another row, or another 16-row block, change the result far beyond rounding."""
    from lyricalignment_amd import ops
    a = _rand(M, K, seed=311, scale=0.5).to(dtype); w = _rand(N, K, seed=312, scale=K ** -0.5).to(dtype)
    bias = _rand(N, seed=313); csum = _rand(N, seed=314)
    m = torch.arange(M)
    mean = torch.where(m % 3 == 0, torch.zeros(M), 100.0 + m.float())
    rstd = torch.where(m % 3 == 0, torch.ones(M), 0.5 + 0.25 * (m % 4).float())
    stats = torch.stack([mean, rstd], dim=1).contiguous()
    ref = rstd.double()[:, None] * (a.double() @ w.double().T - mean.double()[:, None] * csum.double()[None, :]) + bias.double()[None, :]
    ad, wd, bd, cd, sd = a.cuda(), w.cuda(), bias.cuda(), csum.cuda(), stats.cuda()
    old, new = forms(lambda: ops.gemm(ad, wd, bias=bd, ln_stats=sd, ln_csum=cd).clone())
    _same_bits(old, new)
    np.testing.assert_allclose(new.double().cpu().numpy(), ref.numpy(), rtol=1e-2, atol=1e-2)
    old, new = forms(lambda: ops.gemm(ad, wd, ln_stats=sd, ln_csum=cd).clone())      # no bias
    _same_bits(old, new)
    np.testing.assert_allclose(new.double().cpu().numpy(), (ref - bias.double()[None, :]).numpy(), rtol=1e-2, atol=1e-2)
    # GELU of values in the hundreds is the identity or zero; a second set of statistics keeps it in its curved range
    small = torch.stack([torch.where(m % 3 == 0, torch.zeros(M), 0.01 * (m % 50).float()), rstd], dim=1).contiguous()
    refs = small[:, 1].double()[:, None] * (a.double() @ w.double().T - small[:, 0].double()[:, None] * csum.double()[None, :]) + bias.double()[None, :]
    ss = small.cuda()
    old, new = forms(lambda: ops.gemm(ad, wd, bias=bd, gelu=True, ln_stats=ss, ln_csum=cd).clone())
    _same_bits(old, new)
    np.testing.assert_allclose(new.double().cpu().numpy(), torch.nn.functional.gelu(refs).numpy(), rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", KS)
def test_batched_launch_and_row_pitches(K, dtype, forms):
    """z = 3 batch slots with a batch stride beyond M * N; a row pitch wider than N (16-byte rows: the 16-bit staging) and one whose byte pitch
    is no multiple of 16 (the float32 staging's element-wise stores in both settings).  The columns between N and the pitch stay untouched."""
    from lyricalignment_amd import ops
    a, w, bias, ref = _one_hot_operands(K, dtype)
    Z = 3
    az = torch.cat([a * (z + 1) for z in range(Z)], dim=0).contiguous()                 # slot z = (z + 1) x the one-hot rows: still exact
    stride_c = M * N + 24

    def batched():
        out = torch.full((Z * stride_c,), -1.0, dtype=dtype, device="cuda")
        ops.gemm(az, w, out, bias=bias, M=M, lda=K, batch=Z, stride_a=M * K, stride_c=stride_c, ldc=N)
        return out

    old, new = forms(batched)
    _same_bits(old, new)
    for z in range(Z):
        slot = new[z * stride_c:(z + 1) * stride_c].float().cpu()
        want = (z + 1) * (ref - bias.cpu()[None, :]) + bias.cpu()[None, :]               # exact in float32, rounded once to the result type
        assert torch.equal(slot[:M * N].view(M, N), want.to(dtype).float())
        assert torch.all(slot[M * N:] == -1.0)

    for pad in (8, 4):                                                                  # byte pitch 2 (N + 8): 16-byte rows; 2 (N + 4): not
        def pitched():
            out = torch.full((M, N + pad), -1.0, dtype=dtype, device="cuda")
            ops.gemm(a, w, out, bias=bias, gelu=True, M=M, lda=K, ldc=N + pad)
            return out

        old, new = forms(pitched)
        _same_bits(old, new)
        got = new.float().cpu()
        np.testing.assert_allclose(got[:, :N].double().numpy(), torch.nn.functional.gelu(ref.double()).numpy(), rtol=1e-2, atol=1e-2)
        assert torch.all(got[:, N:] == -1.0)
