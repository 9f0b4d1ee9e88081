"""The GEMM kernels (csrc/la_gemm.hip, la_gemm_core.h, la_gemm_pp_kernel.h, la_gemm_pp.h, la_gemm_epilogue.h) against the float64 / int64
restatement of tests/gemm_reference.py, through the C ABI, at the smallest shapes that reach each form.

    form    kernel                                         reached by                                    shapes (M x N [x slots]; K)
    N32     gemm_kernel<float, Cfg<2,2>>  NT               float32 la_gemm                               1x1 127x129 128x128 200x136; 32 64 96 (1-3 ring stages)
    T32     the same, TA|TW / TW / TA                      la_gemm_ex layout flags                       4x4 4x132 132x4 132x132; 1 31 33 77 (partial last stage)
    SK      the same as S batch slots + splitk_reduce      float32, batch 1, few tiles, long K           80x128; 256..2048 (S = 2..16), 257 513 transposed
                                                                                                         (tails 97, 33), 1409x1921x1024 (the S = 4 rule)
    S16     gemm_kernel<bf16|f16, Cfg<2,2>>                option gemm_tile = 128; Mish at any shape      the N32 shapes + 200x38 (nv < 4); 64 128 192
    B16     gemm_kernel<bf16, Cfg<4,3>> three-stage ring   option gemm_tile = 256, >= 512 tiles          513x300x57; 64 128 192 256 (nk = 1..4)
    PP      gemm_pp_kernel, ping-pong loop                 option gemm_tile = 512; K % 128 or K < 256,   529x576; 64 128 192, and 256 with gemm_loop = 99
                                                           or gemm_loop = 99
    PD      gemm_pp_kernel, hand-placed loop               option gemm_tile = 512; K % 128 == 0, >= 256  529x576; 256 384
    ORD     gemm_pp_kernel at its natural routing          la_gemm_fills_chip                            8465x1344 = 34 x 6 tiles; 64 256 (group 5, last group one
                                                                                                         column, M block 32 + a tail of 2 tile rows), 1024 (group 4)
    SPL     gemm_pp_kernel, split-stream epilogue          la_gemm_split (by shape only)                 529x320x32; 64 256.  ln_part: 24337x320; 64
An option is set only where the documented routing would pick another form; la_gemm_fills_chip is asserted for every 16-bit shape, and
every product is one launch of its timer family (gemm_f32 / gemm_bf16).

Exact cases (integer operands in [-3, 3], bias / residual in eighths, integer LayerNorm means, rstd in {0.5, 1, 2}): every partial sum is an
integer below 2^24, so float32 accumulation is exact in any order -- a float32 result must be torch.equal to the reference, a 16-bit result
to the reference rounded once, a split-K result also to the unsplit one.  The split stream's exact cases hold integers of at most 256:
they decode with hi exact and lo == 128.  The expected results have pairwise distinct rows and columns and columns n / n + 4 that differ in
every 16-row block (proved per case in tests/test_host_gemm_kernels.py).

Gaussian cases (GELU, Mish, producer statistics, the lo byte): E32 = max |float32 restatement - float64 restatement| over the case;
    float32 outputs   |got - ref| <= 8 E32
    16-bit outputs    |got - ref| <= ulp_T(ref) / 2 + 8 E32   per element; the default 16-bit GELU + 2.5e-5, gelu="erf" + 1.3e-6 (the
                      header's contract for those forms against erf GELU)
    split stream      round_T(x - 8 E32) <= hi <= round_T(x + 8 E32);  |decode(hi, lo) - x| <= step / 2 + 8 E32
Each comparison prints `form/type case:output err E32 ratio` (16-bit: err is the excess over the rounding and contract terms); the lines of
one MI355X run are kept in profiles/gemm_kernel_errors.txt.  No form needed a term beyond 8 x E32; worst ratios of that run:
    N32 1.04   SK 1.14   S16 1.00   B16 5.57   PP 6.80   PD 2.06   SPL 1.00
The three above 2 are the default 16-bit GELU into bf16 (529x576x128, 513x300x256x57, 529x576x384): the sigmoid fit's own error is 2.53e-5
at x = -0.56, and where ref lies just below a power of two and the kernel's value just above it, the result is rounded on the upper
binade's grid, up to ulp_T(ref) / 2 coarser than the formula grants (7.1e-6 at 2^-8).  gelu="erf" stays below 0.11 on the same cases.

Layout edges (S16, PP, SPL): ldc = N + 1 and N + 2, ldr = N + 1, an output pointer one element off, a batch stride of M ldc + 1, a bias
pointer 4 bytes off.  Every output of every call sits in a sentinel-filled Guard; the bytes between N and the pitch, between slots and
around the allocation must survive.  Operands are ordinary allocations.

The padding behind column K of a K-contiguous operand of the transposed forms (pitch round_up(K, 32)) holds 0.5, NaN or +-Inf: the result
must be the same.  With NaN / Inf this failed for LA_GEMM_TRANS_A alone before compute() masked the W fragments of the partial stage too.
"""
import contextlib
import functools

import pytest
import torch

import gemm_reference as G
from test_gpu_head_kernels import _count_launches
from test_gpu_row_kernels import FACTOR, SLACK, Guard, _L, _ok, _st

pytestmark = pytest.mark.gpu

CASES = G.exact_cases()
T16 = ("bf16", "f16")


class _Out(Guard):
    """A Guard whose view begins `lead` elements behind the slack (an output pointer that lost its alignment); also holds the lo bytes."""

    def __init__(self, shape, strides, dtype, lead=0):
        self.shape, self.strides, self.lead = tuple(shape), tuple(strides), lead
        span = 1 + sum((s - 1) * st for s, st in zip(self.shape, self.strides))
        self.sent = 7.0 if dtype.is_floating_point else 0x5A
        self.buf = torch.full((SLACK + lead + span + SLACK,), self.sent, dtype=dtype, device="cuda")
        self.view = self.buf.as_strided(self.shape, self.strides, SLACK + lead)

    @property
    def ptr(self):
        return self.buf.data_ptr() + (SLACK + self.lead) * self.buf.element_size()

    def check(self, untouched=False):
        torch.cuda.synchronize()
        host = self.buf.cpu()
        keep = torch.ones(host.numel(), dtype=torch.bool)
        if not untouched:
            keep.as_strided(self.shape, self.strides, SLACK + self.lead).fill_(False)
        assert bool((host[keep] == self.sent).all()), "a guard element was overwritten"


@contextlib.contextmanager
def _options(**opts):
    from lyricalignment_amd import _lib
    with contextlib.ExitStack() as st:
        for k, v in opts.items():
            st.enter_context(_lib.option(k, v))
        yield


def _cuda(t, dtype):
    return t.to(dtype).contiguous().cuda()


@functools.lru_cache(maxsize=2)
def _exact_ops(name, dt):
    case = G.exact_case(**CASES[name])
    return case, _cuda(case["a"], G.TYPES[dt]), _cuda(case["w"], G.TYPES[dt]), _cuda(case["bias"], torch.float32)


@functools.lru_cache(maxsize=2)
def _gauss_ops(M, N, K, batch, dt):
    g = G.gauss_case(M, N, K, batch, dt)
    return g, g["a"].cuda(), g["w"].cuda(), g["bias"].cuda()


def _pitched_rows(t, pitch):
    """t [.., R, C] float64 -> device float32 [.., R, pitch], pad columns zero."""
    buf = torch.zeros(t.shape[:-1] + (pitch,), dtype=torch.float32)
    buf[..., :t.shape[-1]] = t.float()
    return buf.cuda()


def _gemm(dt, a, w, M, N, K, batch, *, out, bias=None, act=None, erf=False, residual=None, inplace=False, stats=None, csum=None,
          producer=False, part=False, ldc=None, ldr=None, lead=0, skew=0):
    """One la_gemm / la_gemm_fused_ln call.  a [Z, M, K], w [N, K] device tensors of the type; bias: device float32 (a view keeps its own
    pointer); residual: float64 [Z, M, N] on the CPU (inplace: it is the initial content of C).  -> {'c', 'c16', 'part'} on the CPU."""
    L = _L()
    T = G.TYPES[dt]
    ldc = N if ldc is None else ldc
    sc = M * ldc + skew
    c = _Out((batch, M, N), (sc, ldc, 1), torch.float32 if out == "f32" else T, lead)
    epi = (G.EPI_BIAS if bias is not None else 0) | (G.EPI_OUT_F32 if out == "f32" and dt != "f32" else 0)
    if act == "gelu":
        epi |= G.EPI_GELU | (G.EPI_GELU_ERF if erf else 0)
    elif act == "mish":
        epi |= G.EPI_MISH
    rp, rl, rs, rbuf = 0, 0, 0, None
    if inplace:
        assert out == "f32"
        c.set(residual.float().cuda())
        rp, rl, rs = c.ptr, ldc, sc
    elif residual is not None:
        rl = N if ldr is None else ldr
        rbuf = _pitched_rows(residual, rl)
        rp, rs = rbuf.data_ptr(), M * rl
    if rp:
        epi |= G.EPI_RESIDUAL
    bp = bias.data_ptr() if bias is not None else 0
    c2 = _Out((batch, M, N), (sc, ldc, 1), T, 0) if producer else None
    pt = _Out((N // 64, M, 2), (2 * M, 2, 1), torch.float32) if part else None
    sd = _cuda(stats, torch.float32) if stats is not None else None
    cd = _cuda(csum, torch.float32) if csum is not None else None
    with _count_launches("gemm_f32" if dt == "f32" else "gemm_bf16") as cnt:
        if producer or sd is not None:
            _ok(L.la_gemm_fused_ln(G.CODES[dt], M, N, K, batch, a.data_ptr(), K, M * K, w.data_ptr(), c.ptr, ldc, sc, bp, rp, rl, rs, epi,
                                   c2.ptr if c2 else 0, ldc if c2 else 0, sc if c2 else 0, sd.data_ptr() if sd is not None else 0,
                                   cd.data_ptr() if cd is not None else 0, pt.ptr if pt else 0, _st()), "la_gemm_fused_ln")
        else:
            _ok(L.la_gemm(G.CODES[dt], M, N, K, batch, a.data_ptr(), K, M * K, w.data_ptr(), c.ptr, ldc, sc, bp, rp, rl, rs, epi, _st()), "la_gemm")
    assert cnt.n == 1, f"{cnt.n} launches"
    res = {"c": c.get().double()}
    c.check()
    if c2:
        res["c16"] = c2.get().double()
        c2.check()
    if pt:
        res["part"] = pt.get().double()
        pt.check()
    return res


def _exact(what, got, want):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    if bool(bad.any()):
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {idx}: got {float(got[tuple(idx)])}, "
                             f"want {float(want[tuple(idx)])}")


def _measured(form, dt, case, output, got, ref, e32, out="f32", extra=0.0):
    """|got - ref| <= [ulp_T(ref) / 2 + extra +] 8 E32 per element; prints the figures first."""
    d = (got - ref).abs()
    if out != "f32":
        d = d - 0.5 * G.ulp_T(ref, out) - extra
    err = float(d.max())
    err = max(err, 0.0) if err == err else err
    ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{form}/{dt} {case}:{output} {err:.3e} {e32:.3e} {ratio:.2f}")
    assert err <= FACTOR * e32, (form, dt, case, output, err, e32)


def _fills(M, N, batch=1):
    got = bool(_L().la_gemm_fills_chip(M, N, batch))
    assert got == G.fills_chip(M, N, batch)
    return got


def _gauss_runs(form, dt, M, N, K, batch, outs, acts, **kw):
    """The measured activations of one form on a Gaussian case: bias, activation, f32 residual."""
    g, a, w, b = _gauss_ops(M, N, K, batch, dt)
    for out in outs:
        for act, erf in acts:
            if erf and out == "f32":
                continue
            r64, e = G.gauss_ref(g, bias=g["bias"], act=act, residual=g["residual"])
            got = _gemm(dt, a, w, M, N, K, batch, out=out, bias=b, act=act, erf=erf, residual=g["residual"], **kw)["c"]
            extra = 0.0 if out == "f32" or act != "gelu" else (G.GELU_ERF_ABS if erf else G.GELU_SIG_ABS)
            _measured(form, dt, f"{M}x{N}x{K}" + (f"x{batch}" if batch > 1 else ""), f"{act}{'_erf' if erf else ''}->{out}", got, r64, e, out, extra)


ACTS32 = (("gelu", False), ("mish", False))
ACTS16 = (("gelu", False), ("gelu", True), ("mish", False))


# ---- N32: float32, both operands K-contiguous ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", G.F32_K)
@pytest.mark.parametrize("M,N", G.MN_SMALL)
def test_f32_nt_is_the_int64_product(M, N, K):
    case, a, w, b = _exact_ops(f"f32nt_{M}x{N}x{K}", "f32")
    assert G.splitk_plan(M, N, K)[0] == 1
    run = functools.partial(_gemm, "f32", a, w, M, N, K, 1, out="f32")
    _exact("plain", run()["c"], G.expected(case, "plain", "f32"))
    _exact("bias, ldc = N + 1", run(bias=b, ldc=N + 1)["c"], G.expected(case, "bias", "f32"))
    _exact("residual, ldr = N + 1", run(bias=b, residual=case["residual"], ldr=N + 1)["c"], G.expected(case, "res", "f32"))
    _exact("residual in place, ldc = N + 3", run(bias=b, residual=case["residual"], inplace=True, ldc=N + 3)["c"], G.expected(case, "res", "f32"))
    if (M, N) == (200, 136):
        _gauss_runs("N32", "f32", M, N, K, 1, ("f32",), ACTS32)


# ---- T32: transposed operands -------------------------------------------------------------------------------------------------------

def _fill(shape, kind):
    if kind == "inf":
        sign = 1.0 - 2.0 * (torch.arange(shape[-1]) % 2).float()
        return (sign * float("inf")).expand(shape).clone()
    return torch.full(shape, float("nan") if kind == "nan" else 0.5)


def _padded(t, pitch, kind):
    """t [R, C] float64 -> device float32 [R, pitch] whose pad columns hold 0.5, NaN or +-Inf."""
    buf = _fill((t.shape[0], pitch), kind)
    buf[:, :t.shape[1]] = t.float()
    return buf.cuda()


def _gemm_ex(layout, a, w, M, N, K, *, pad, bias=None, act=None):
    """la_gemm_ex on float32 operands a [M, K], w [N, K] (float64, CPU) stored in `layout`: 'tt' both [K][rows] (pitch rows + 4), 'tw' A
    K-contiguous with pitch round_up(K, 32) and W [K][N + 4], 'ta' the other way round."""
    L = _L()
    kp = G.round_up(K, 32)
    ta, tw = layout in ("tt", "ta"), layout in ("tt", "tw")
    ad = _padded(a.T.contiguous(), M + 4, pad) if ta else _padded(a, kp, pad)
    wd = _padded(w.T.contiguous(), N + 4, pad) if tw else _padded(w, kp, pad)
    c = _Out((M, N), (N, 1), torch.float32)
    epi = (G.TRANS_A if ta else 0) | (G.TRANS_W if tw else 0) | (G.EPI_BIAS if bias is not None else 0) | (G.EPI_GELU if act == "gelu" else 0)
    with _count_launches("gemm_f32") as cnt:
        _ok(L.la_gemm_ex(0, M, N, K, 1, ad.data_ptr(), ad.stride(0), 0, wd.data_ptr(), wd.stride(0), 0, c.ptr, N, 0,
                         bias.data_ptr() if bias is not None else 0, epi, _st()), "la_gemm_ex")
    assert cnt.n == 1
    got = c.get().double()
    c.check()
    return got


@pytest.mark.parametrize("pad", ["half", "nan", "inf"])
@pytest.mark.parametrize("K", G.TRANS_K)
@pytest.mark.parametrize("layout", ["tt", "tw", "ta"])
def test_f32_transposed_forms_ignore_what_lies_behind_column_k(layout, K, pad):
    for M, N in G.trans_shapes(K):
        case = G.exact_case(**CASES[f"trans_{M}x{N}x{K}"])
        b = _cuda(case["bias"], torch.float32)
        a, w = case["a"][0], case["w"]
        _exact(f"{layout} {M}x{N}x{K} plain, pad {pad}", _gemm_ex(layout, a, w, M, N, K, pad=pad), G.expected(case, "plain", "f32")[0])
        _exact(f"{layout} {M}x{N}x{K} bias, pad {pad}", _gemm_ex(layout, a, w, M, N, K, pad=pad, bias=b), G.expected(case, "bias", "f32")[0])


# ---- SK: float32 split-K ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K,S", G.SPLITK_NT)
def test_f32_split_k_is_exact_and_equals_the_unsplit_product(M, N, K, S):
    case, a, w, b = _exact_ops(f"splitk_{M}x{N}x{K}", "f32")
    assert G.splitk_plan(M, N, K)[0] == S
    run = functools.partial(_gemm, "f32", a, w, M, N, K, 1, out="f32")
    forms = (("plain", dict(), "plain"), ("bias", dict(bias=b, ldc=N + 1), "bias"), ("residual", dict(bias=b, residual=case["residual"], ldr=N + 1), "res"),
             ("in place", dict(bias=b, residual=case["residual"], inplace=True), "res"))
    for what, kw, name in forms:
        split = run(**kw)["c"]
        with _options(gemm_splitk=0):
            whole = run(**kw)["c"]
        _exact(f"{what}, S = {S}", split, G.expected(case, name, "f32"))
        _exact(f"{what}, unsplit", whole, G.expected(case, name, "f32"))
    # GELU of exact sums: the two plans hand the same float32 value to the same function
    split = run(bias=b, act="gelu", residual=case["residual"])["c"]
    with _options(gemm_splitk=0):
        whole = run(bias=b, act="gelu", residual=case["residual"])["c"]
    _exact("gelu split against unsplit", split, whole)
    if M == 80:
        _gauss_runs("SK", "f32", M, N, K, 1, ("f32",), ACTS32)


@pytest.mark.parametrize("pad", ["half", "nan"])
@pytest.mark.parametrize("M,N,K,S", G.SPLITK_T)
@pytest.mark.parametrize("layout", ["tt", "tw", "ta"])
def test_f32_split_k_with_a_short_last_slot(layout, M, N, K, S, pad):
    case = G.exact_case(**CASES[f"splitk_t_{M}x{N}x{K}"])
    s, kc, tail = G.splitk_plan(M, N, K)
    assert s == S and tail < kc and tail % 32 != 0
    b = _cuda(case["bias"], torch.float32)
    a, w = case["a"][0], case["w"]
    split = _gemm_ex(layout, a, w, M, N, K, pad=pad, bias=b)
    with _options(gemm_splitk=0):
        whole = _gemm_ex(layout, a, w, M, N, K, pad=pad, bias=b)
    _exact(f"{layout} S = {S}", split, G.expected(case, "bias", "f32")[0])
    _exact(f"{layout} unsplit", whole, G.expected(case, "bias", "f32")[0])
    _exact(f"{layout} plain", _gemm_ex(layout, a, w, M, N, K, pad=pad), G.expected(case, "plain", "f32")[0])
    gelu = _gemm_ex(layout, a, w, M, N, K, pad=pad, bias=b, act="gelu")                  # exact sums: both plans hand GELU the same value
    with _options(gemm_splitk=0):
        _exact(f"{layout} gelu split against unsplit", gelu, _gemm_ex(layout, a, w, M, N, K, pad=pad, bias=b, act="gelu"))

# ---- S16: the 128 x 128 kernel on 16-bit operands -----------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N", G.MN_SMALL + ((200, 38),))
@pytest.mark.parametrize("dt", T16)
def test_small_tile_16_bit(dt, M, N):
    for K in G.S16_K:
        case, a, w, b = _exact_ops(f"s16_{M}x{N}x{K}", dt)
        with _options(gemm_tile=128):
            for out in ("f32", dt):
                run = functools.partial(_gemm, dt, a, w, M, N, K, 1, out=out)
                _exact(f"K={K} plain -> {out}", run()["c"], G.expected(case, "plain", out))
                _exact(f"K={K} bias -> {out}", run(bias=b)["c"], G.expected(case, "bias", out))
                _exact(f"K={K} residual -> {out}", run(bias=b, residual=case["residual"])["c"], G.expected(case, "res", out))
            _exact(f"K={K} in place", _gemm(dt, a, w, M, N, K, 1, out="f32", bias=b, residual=case["residual"], inplace=True)["c"],
                   G.expected(case, "res", "f32"))
            if M == 200:
                _gauss_runs("S16", dt, M, N, K, 1, ("f32", dt), ACTS16)


@pytest.mark.parametrize("dt", T16)
def test_mish_keeps_a_chip_filling_shape_on_the_small_tile(dt):
    """200 x 136 x 192 slots fills the chip (192 tiles of 256 x 256), and the 256 x 256 kernel has no Mish: the product stays on the 128 x 128
    kernel, whose result carries the activation."""
    M, N, K, Z = 200, 136, 64, 192
    assert _fills(M, N, Z) and not _fills(M, N, Z - 1)
    _gauss_runs("S16", dt, M, N, K, Z, ("f32", dt), (("mish", False),))


# ---- B16: the 256 x 128 three-stage ring --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", G.BIG_K)
def test_three_stage_ring(K):
    M, N, Z = G.BIG_SHAPE
    case, a, w, b = _exact_ops(f"big_{K}", "bf16")
    assert G.cdiv(M, 256) * G.cdiv(N, 128) * Z >= 512
    with _options(gemm_tile=256):
        for out in ("f32", "bf16"):
            run = functools.partial(_gemm, "bf16", a, w, M, N, K, Z, out=out)
            _exact(f"plain -> {out}", run()["c"], G.expected(case, "plain", out))
            _exact(f"bias -> {out}", run(bias=b)["c"], G.expected(case, "bias", out))
            _exact(f"residual -> {out}", run(bias=b, residual=case["residual"])["c"], G.expected(case, "res", out))
        if K == 256:
            _gauss_runs("B16", "bf16", M, N, K, Z, ("f32", "bf16"), ACTS16[:2])


# ---- PP / PD: the 256 x 256 kernel, forced ------------------------------------------------------------------------------------------

def _consumer_runs(form, dt, M, N, K, outs, **kw):
    g, a, w, b = _gauss_ops(M, N, K, 1, dt)
    for out in outs:
        for act, erf in ((None, False), ("gelu", False), ("gelu", True)):
            if erf and out == "f32":
                continue
            r64, e = G.gauss_ref(g, bias=g["bias"], act=act, stats=g["stats"], csum=g["csum"])
            got = _gemm(dt, a, w, M, N, K, 1, out=out, bias=b, act=act, erf=erf, stats=g["stats"], csum=g["csum"], **kw)["c"]
            extra = 0.0 if out == "f32" or act != "gelu" else (G.GELU_ERF_ABS if erf else G.GELU_SIG_ABS)
            _measured(form, dt, f"{M}x{N}x{K}", f"ln_{act}{'_erf' if erf else ''}->{out}", got, r64, e, out, extra)


def _producer_runs(form, dt, M, N, K):
    """out16 = the f32 result rounded once; ln_part = (mean, M2) of each 64-column segment of the rows out16 holds (driven: the statistics
    are compared with the float64 statistics of the kernel's own 16-bit copy, so a rounding flip of the copy is not their error)."""
    g, a, w, b = _gauss_ops(M, N, K, 1, dt)
    r64, e = G.gauss_ref(g, bias=g["bias"], residual=g["residual"])
    got = _gemm(dt, a, w, M, N, K, 1, out="f32", bias=b, residual=g["residual"], producer=True, part=True)
    _measured(form, dt, f"{M}x{N}x{K}", "producer->f32", got["c"], r64, e)
    _measured(form, dt, f"{M}x{N}x{K}", f"producer->out16", got["c16"], r64, e, dt)
    _exact("out16 is the f32 result rounded once", got["c16"], G.round_T(got["c"], dt))
    s64, s32 = G.segment_stats(got["c16"][0]), G.segment_stats(got["c16"][0], torch.float32)
    for i, which in enumerate(("mean", "m2")):
        _measured(form, dt, f"{M}x{N}x{K}", f"ln_part.{which}", got["part"][..., i], s64[..., i], G.e32(s32[..., i], s64[..., i]))


@pytest.mark.parametrize("K,loop", [(64, 0), (128, 0), (192, 0), (256, 99), (256, 0), (384, 0)])
@pytest.mark.parametrize("dt", T16)
def test_big_tile_forced(dt, K, loop):
    M, N = G.PP_SHAPE
    form = "PD" if K % 128 == 0 and K >= 256 and loop != 99 else "PP"
    case, a, w, b = _exact_ops(f"pp_{K}", dt)
    assert not _fills(M, N)
    res, st, cs = case["residual"], case["stats"], case["csum"]
    with _options(gemm_tile=512, gemm_loop=loop):
        for out, epi16 in (("f32", 1), (dt, 0), (dt, 1)):
            with _options(gemm_epi16=epi16):
                run = functools.partial(_gemm, dt, a, w, M, N, K, 1, out=out)
                tag = f"{form} K={K} -> {out} epi16={epi16}: "
                _exact(tag + "plain", run()["c"], G.expected(case, "plain", out))
                _exact(tag + "bias", run(bias=b)["c"], G.expected(case, "bias", out))
                _exact(tag + "residual", run(bias=b, residual=res)["c"], G.expected(case, "res", out))
                _exact(tag + "consumer", run(stats=st, csum=cs)["c"], G.expected(case, "ln", out))
                _exact(tag + "consumer + bias", run(bias=b, stats=st, csum=cs)["c"], G.expected(case, "ln_bias", out))
                if out == "f32":
                    _exact(tag + "in place", run(bias=b, residual=res, inplace=True)["c"], G.expected(case, "res", out))
                    for name, kw in (("bias", dict(bias=b)), ("res", dict(bias=b, residual=res)), ("res", dict(bias=b, residual=res, inplace=True))):
                        got = run(producer=True, part=True, **kw)
                        _exact(tag + f"producer {name}", got["c"], G.expected(case, name, "f32"))
                        _exact(tag + f"producer {name} out16", got["c16"], G.expected(case, name, dt))
                _gauss_runs(form, dt, M, N, K, 1, (out,), ACTS16[:2])
                _consumer_runs(form, dt, M, N, K, (out,))
        _producer_runs(form, dt, M, N, K)


# ---- ORD: the tile order at natural routing -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,dt", [(64, "bf16"), (256, "bf16"), (1024, "bf16"), (64, "f16")])
def test_tile_order_of_34_by_6_tiles(K, dt):
    """Every element of 8465 x 1344 at the kernel's own routing: the tile a workgroup computes is the tile whose A rows, W rows, bias, row
    statistics and C addresses it uses."""
    M, N = G.ORDER_SHAPE
    case, a, w, b = _exact_ops(f"order_{K}", dt)
    assert _fills(M, N) and G.pp_group(N, K) == ((5, 32) if K < 1024 else (4, 32))
    out16 = dt if dt in case["outs"] else "f32"
    _exact("bias -> f32", _gemm(dt, a, w, M, N, K, 1, out="f32", bias=b)["c"], G.expected(case, "bias", "f32"))
    _exact(f"consumer + bias -> {out16}", _gemm(dt, a, w, M, N, K, 1, out=out16, bias=b, stats=case["stats"], csum=case["csum"])["c"],
           G.expected(case, "ln_bias", out16))


# ---- SPL: the split residual stream -------------------------------------------------------------------------------------------------

def _split(dt, a, w, M, N, K, batch, *, bias=None, gelu=False, residual=None, shared=False, stream=None, part=False, ld=None, ldr=None,
           lead=0, skew=0):
    """One la_gemm_split call.  residual: float64 [Z, M, N] f32 rows ([M, N] with shared: stride_r = 0); stream: (hi, lo) CPU tensors [Z, M, N]
    = the initial stream of the in-place form.  -> (hi as float64, lo as int64, decode(hi, lo) by ops.split_decode, ln_part)."""
    from lyricalignment_amd import ops
    L = _L()
    T = G.TYPES[dt]
    ld = N if ld is None else ld
    sc = M * ld + skew
    hi, lo = _Out((batch, M, N), (sc, ld, 1), T, lead), _Out((batch, M, N), (sc, ld, 1), torch.uint8, lead)
    epi = (G.EPI_BIAS if bias is not None else 0) | (G.EPI_GELU if gelu else 0)
    rp, rl, rs, rbuf = 0, 0, 0, None
    if stream is not None:
        hi.set(stream[0].cuda())
        lo.set(stream[1].cuda())
        epi |= G.EPI_RESIDUAL
    elif residual is not None:
        rl = N if ldr is None else ldr
        rbuf = _pitched_rows(residual, rl)
        rp, rs = rbuf.data_ptr(), (0 if shared else M * rl)
        epi |= G.EPI_RESIDUAL
    pt = _Out((N // 64, M, 2), (2 * M, 2, 1), torch.float32) if part else None
    with _count_launches("gemm_bf16") as cnt:
        _ok(L.la_gemm_split(G.CODES[dt], M, N, K, batch, a.data_ptr(), K, M * K, w.data_ptr(), hi.ptr, lo.ptr, ld, sc,
                            bias.data_ptr() if bias is not None else 0, rp, rl, rs, epi, pt.ptr if pt else 0, _st()), "la_gemm_split")
    assert cnt.n == 1
    torch.cuda.synchronize()
    dec = ops.split_decode(hi.view.contiguous(), lo.view.contiguous()).double().cpu()
    h, l = hi.get(), lo.get()
    hi.check()
    lo.check()
    p = None
    if pt:
        p = pt.get().double()
        pt.check()
    return h.double(), l.to(torch.int64), dec, p


def _split_exact(what, got, x):
    """An integer of at most 256 is a value of both 16-bit types: hi is x itself, lo says 'no remainder', the decoder returns x."""
    assert float(x.abs().max()) <= 256 and bool((x == x.round()).all())
    _exact(what + " hi", got[0], x)
    assert bool((got[1] == 128).all()), f"{what}: {int((got[1] != 128).sum())} lo bytes are not 128"
    _exact(what + " decode", got[2], x)


def _split_measured(dt, case, output, got, x64, e):
    hi, lo, dec, _ = got
    assert bool((hi >= G.round_T(x64 - FACTOR * e, dt)).all()) and bool((hi <= G.round_T(x64 + FACTOR * e, dt)).all()), (case, output, "hi")
    step = G.split_step(hi, dt)
    err = max(float(((dec - x64).abs() - 0.5 * step).max()), 0.0)
    print(f"SPL/{dt} {case}:{output} {err:.3e} {e:.3e} {err / e:.2f}")
    assert err <= FACTOR * e, (case, output, err, e)
    assert bool(((lo >= 1) & (lo <= 255)).all())


@pytest.mark.parametrize("K", G.SPLIT_K)
@pytest.mark.parametrize("dt", T16)
def test_split_stream(dt, K):
    M, N, Z = G.SPLIT_SHAPE
    case, a, w, b = _exact_ops(f"split_{K}", dt)
    assert _fills(M, N, Z)
    res = case["residual"]
    _split_exact("plain", _split(dt, a, w, M, N, K, Z), case["ref"]["plain"])
    _split_exact("bias", _split(dt, a, w, M, N, K, Z, bias=b), case["ref"]["bias"])
    _split_exact("stem: f32 rows, stride_r = 0", _split(dt, a, w, M, N, K, Z, bias=b, residual=res[0], shared=True), case["ref"]["bias"] + res[0][None])
    stream = (res.to(G.TYPES[dt]), torch.full(res.shape, 128, dtype=torch.uint8))
    _split_exact("in place", _split(dt, a, w, M, N, K, Z, bias=b, stream=stream), case["ref"]["res"])
    # Gaussian: the lo byte carries a remainder
    g, ga, gw, gb = _gauss_ops(M, N, K, Z, dt)
    name = f"{M}x{N}x{K}x{Z}"
    for gelu in (False, True):
        act = "gelu" if gelu else None
        x64, e = G.gauss_ref(g, bias=g["bias"], act=act, residual=g["residual"][0][None])
        _split_measured(dt, name, f"stem{'_gelu' if gelu else ''}", _split(dt, ga, gw, M, N, K, Z, bias=gb, gelu=gelu, residual=g["residual"][0], shared=True), x64, e)
        h0, l0 = G.split_encode(g["residual"].double(), dt)
        x0 = G.split_decode(h0, l0, dt)
        x64 = G.epilogue(g["acc64"], bias=g["bias"].double(), act=act, residual=x0)
        x32 = G.epilogue(g["acc32"], bias=g["bias"], act=act, residual=x0.float())
        _split_measured(dt, name, f"in_place{'_gelu' if gelu else ''}", _split(dt, ga, gw, M, N, K, Z, bias=gb, gelu=gelu, stream=(h0, l0)), x64, G.e32(x32, x64))


@pytest.mark.parametrize("dt", T16)
def test_split_stream_partial_statistics(dt):
    """ln_part takes batch 1, so the rows alone must make 192 tiles: 96 x 2 tiles of 256 x 256, the last row tile 17 rows deep."""
    M, N, K = 95 * 256 + 17, 320, 64
    assert _fills(M, N) and not _fills(M - 17, N)
    g, a, w, b = _gauss_ops(M, N, K, 1, dt)
    x64, e = G.gauss_ref(g, bias=g["bias"], residual=g["residual"])
    got = _split(dt, a, w, M, N, K, 1, bias=b, residual=g["residual"], part=True)
    _split_measured(dt, f"{M}x{N}x{K}", "stem", got, x64, e)
    s64, s32 = G.segment_stats(got[0][0]), G.segment_stats(got[0][0], torch.float32)
    for i, which in enumerate(("mean", "m2")):
        _measured("SPL", dt, f"{M}x{N}x{K}", f"ln_part.{which}", got[3][..., i], s64[..., i], G.e32(s32[..., i], s64[..., i]))


# ---- layout edges -------------------------------------------------------------------------------------------------------------------

EDGES = {"ldc+1": dict(ldc=1), "ldc+2": dict(ldc=2), "ldr+1": dict(ldr=1), "pointer+1": dict(lead=1), "slot+1": dict(skew=1), "bias+4B": dict()}


def _shifted_bias(b):
    buf = torch.zeros(b.numel() + 1, dtype=torch.float32, device="cuda")
    buf[1:] = b
    assert buf[1:].data_ptr() % 16 == 4
    return buf[1:]


@pytest.mark.parametrize("edge", sorted(EDGES))
@pytest.mark.parametrize("kernel", ["S16", "PP"])
@pytest.mark.parametrize("dt", T16)
def test_layout_edges_of_the_16_bit_kernels(dt, kernel, edge):
    name = "edge_200x136x64" if kernel == "S16" else "edge_pp_529x576x64"
    case, a, w, b = _exact_ops(name, dt)
    M, N, K, Z = case["M"], case["N"], case["K"], case["batch"]
    kw = {k: (N + v if k in ("ldc", "ldr") else v) for k, v in EDGES[edge].items()}
    bias = _shifted_bias(b) if edge == "bias+4B" else b
    with _options(gemm_tile=128 if kernel == "S16" else 512):
        for out in (dt, "f32"):
            _exact(f"{kernel} {edge} residual -> {out}", _gemm(dt, a, w, M, N, K, Z, out=out, bias=bias, residual=case["residual"], **kw)["c"],
                   G.expected(case, "res", out))
            if "ldr" not in kw:
                _exact(f"{kernel} {edge} bias -> {out}", _gemm(dt, a, w, M, N, K, Z, out=out, bias=bias, **kw)["c"], G.expected(case, "bias", out))


@pytest.mark.parametrize("edge", sorted(EDGES))
@pytest.mark.parametrize("dt", T16)
def test_layout_edges_of_the_split_stream(dt, edge):
    M, N, Z = G.SPLIT_SHAPE
    K = 64
    case, a, w, b = _exact_ops(f"split_{K}", dt)
    kw = {("ld" if k == "ldc" else k): (N + v if k in ("ldc", "ldr") else v) for k, v in EDGES[edge].items()}
    bias = _shifted_bias(b) if edge == "bias+4B" else b
    res = case["residual"]
    _split_exact(f"{edge} f32 rows", _split(dt, a, w, M, N, K, Z, bias=bias, residual=res, **kw), case["ref"]["res"])
    if "ldr" not in kw:
        stream = (res.to(G.TYPES[dt]), torch.full(res.shape, 128, dtype=torch.uint8))
        _split_exact(f"{edge} in place", _split(dt, a, w, M, N, K, Z, bias=bias, stream=stream, **kw), case["ref"]["res"])
