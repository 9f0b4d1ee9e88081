"""Plain restatement of the GEMM family (csrc/la_gemm.hip, la_gemm_pp_kernel.h, la_gemm_epilogue.h) on the CPU in float64 / int64: case
generators, the epilogues in the order the kernels apply them (LayerNorm fold or bias, activation, residual), the producer's 16-bit copy
with its per-64-column (mean, M2), and the split residual stream's encoding (ops.split_decode is the decoder).

Exact cases: operands are seeded integers in [-3, 3] (exact in bf16, f16 and float32), bias and residual multiples of 1/8, LayerNorm
statistics integer means with rstd in {0.5, 1, 2} and integer column sums.  Every partial sum of every product is an integer below 2^24, so
a float32 accumulator holds it exactly whatever the order: any k order, any ring, any split-K plan gives the same bits, and the expected
result is the int64 product.  A generated case also has pairwise distinct rows, pairwise distinct columns, and columns n and n + 4 that
differ inside every 16-row block, so a misplaced row, quad or tile cannot reproduce it; the generator moves to the next seed until all of
that holds (tests/test_host_gemm_kernels.py proves it per case).

Gaussian cases: a ~ N(0, 1), w ~ N(0, 1 / K) rounded to the operand type, bias ~ N(0, 0.5^2), residual ~ N(0, 1).  The yardstick is
E32 = max |float32 restatement - float64 restatement| over the case.
"""
import functools

import torch

TYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CODES = {"f32": 0, "bf16": 1, "f16": 2}
EPI_BIAS, EPI_GELU, EPI_RESIDUAL, EPI_OUT_F32, EPI_MISH, EPI_GELU_ERF = 1, 2, 4, 8, 16, 4096
TRANS_A, TRANS_W = 512, 1024
SPLIT_SH = {"bf16": 16, "f16": 19}            # la_common.h SplitRes<T>::SH
SPLIT_EMIN = {"bf16": -200, "f16": -13}       # SplitRes<T>::EMIN (frexp exponent floor)
GELU_SIG_ABS, GELU_ERF_ABS = 2.5e-5, 1.3e-6   # include/lyricalign.h LA_EPI_GELU / LA_EPI_GELU_ERF, 16-bit results
FILL_TILES = 192                              # la_gemm_params.h
ROW_BLOCK = 16


def _g(seed):
    return torch.Generator().manual_seed(int(seed))


def round_up(x, m):
    return (x + m - 1) // m * m


def cdiv(a, b):
    return (a + b - 1) // b


# ---- routing arithmetic (restated from la_gemm.hip / la_gemm_params.h / la_gemm_core.h) ---------------------------------------------

def fills_chip(M, N, batch=1):
    return N > 128 and cdiv(M, 256) * cdiv(N, 256) * batch >= FILL_TILES


def splitk_plan(M, N, K):
    """(S, Kc, K_tail) of a float32 batch-1 product; S = 1: no split."""
    tiles, ksteps = cdiv(M, 128) * cdiv(N, 128), cdiv(K, 32)
    S = 1
    while S < 16 and tiles * S * 2 <= 256 and ksteps // (S * 2) >= 4:
        S *= 2
    if S == 1 and K >= 1024 and M * N <= (4 << 20):
        if tiles * 4 % 256 == 0 and tiles % 256 != 0 and tiles < 256:
            S = 4
        elif tiles * 2 % 256 == 0 and tiles % 256 != 0 and tiles < 512:
            S = 2
    if S == 1:
        return 1, K, K
    Kc = cdiv(ksteps, S) * 32
    if K - (S - 1) * Kc <= 0:
        S = cdiv(K, Kc)
    return S, Kc, K - (S - 1) * Kc


def pp_group(N, K):
    """Column tiles per group of the 256 x 256 kernel's tile order, and its M block (0 = none)."""
    t128, tn = cdiv(N, 128), cdiv(N, 256)
    g = max(1, min(16, (2 << 20) // (128 * K * 2)))
    group = min(tn, max(4, min(g, t128) // 2))
    return group, (32 if tn > group else 0)


def tile_coord_mb(tile, tiles_m, tiles_n, group, mblock):
    if mblock <= 0:
        per_group = group * tiles_m
        g = tile // per_group
        gw = min(group, tiles_n - g * group)
        rem = tile - g * per_group
        return rem // gw, g * group + rem % gw
    per_block = mblock * tiles_n
    b, nb, rows = tile // per_block, tiles_m // mblock, mblock
    if b >= nb:
        b, rows = nb, tiles_m - nb * mblock
    off = tile - b * per_block
    g = off // (rows * group)
    gw = min(group, tiles_n - g * group)
    rem = off - g * rows * group
    return b * mblock + rem // gw, g * group + rem % gw


# ---- number formats -----------------------------------------------------------------------------------------------------------------

def ulp_T(ref, dt):
    """Spacing of the 16-bit type `dt` at |ref| (float64), subnormal range included."""
    mant, emin = {"bf16": (7, -126), "f16": (10, -14)}[dt]
    _, e = torch.frexp(ref.double().abs())
    e = torch.where(ref == 0, torch.full_like(e, emin), e - 1).clamp(min=emin)
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e - mant)


def round_T(x, dt):
    """x (float64) rounded once to the type, as float64."""
    return x.double().to(TYPES[dt]).double() if dt != "f32" else x.double().float().double()


# ---- epilogues ----------------------------------------------------------------------------------------------------------------------

def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * (0.5 ** 0.5)))


def mish(x):
    return x * torch.tanh(torch.log1p(torch.exp(-x.abs())) + x.clamp(min=0))


def epilogue(acc, *, bias=None, act=None, residual=None, stats=None, csum=None):
    """acc [.., M, N] in float64 or float32 -> the result in the same precision, operations in the kernels' order:
    LayerNorm consumer rstd (acc - mean c) + b (stats [M, 2] = (mean, rstd), csum [N]) or + bias; GELU (erf) / Mish; + residual."""
    dt = acc.dtype
    v = acc
    if stats is not None:
        mean, rstd = stats[:, 0].to(dt)[:, None], stats[:, 1].to(dt)[:, None]
        v = rstd * (v - mean * csum.to(dt)[None, :])
    if bias is not None:
        v = v + bias.to(dt)
    if act == "gelu":
        v = gelu(v)
    elif act == "mish":
        v = mish(v)
    if residual is not None:
        v = v + residual.to(dt)
    return v


def product(a, w, dtype=torch.float64):
    """a [Z, M, K] x w [N, K] -> [Z, M, N]"""
    return a.to(dtype) @ w.to(dtype).T


def product_int64(a, w):
    return a.to(torch.int64) @ w.to(torch.int64).T


def segment_stats(x16, dtype=torch.float64):
    """x16 [M, N] values of the 16-bit copy, N % 64 == 0 -> [N / 64, M, 2] = (mean, sum of squared deviations) per 64-column segment."""
    M, N = x16.shape
    s = x16.to(dtype).reshape(M, N // 64, 64)
    mean = s.mean(-1)
    m2 = ((s - mean[..., None]) ** 2).sum(-1)
    return torch.stack([mean, m2], -1).permute(1, 0, 2).contiguous()


def stats_finalize(part, eps=1e-5, dtype=torch.float64):
    """[slots, M, 2] -> [M, 2] (mean, rstd): equal-sized groups combined (Chan et al.)."""
    p = part.to(dtype)
    slots = p.shape[0]
    mean = p[..., 0].mean(0)
    m2 = (p[..., 1] + 64.0 * (p[..., 0] - mean[None]) ** 2).sum(0)
    return torch.stack([mean, 1.0 / torch.sqrt(m2 / (64.0 * slots) + eps)], -1)


# ---- split residual stream ----------------------------------------------------------------------------------------------------------

def split_exponent(hi16, dt):
    """frexp exponent of hi as SplitRes uses it (f16 subnormals share the smallest normal binade's)."""
    _, e = torch.frexp(hi16.double())
    return e.clamp(min=SPLIT_EMIN[dt]) if dt == "f16" else e


def split_step(hi16, dt):
    """The lo step at hi: (128 / 127) 2^(e - SH) = ulp(hi) / 254."""
    e = split_exponent(hi16, dt)
    return (128.0 / 127.0) * torch.ldexp(torch.ones_like(e, dtype=torch.float64), e - SPLIT_SH[dt])


def split_encode(x, dt):
    """x (float64) -> (hi in the type, lo uint8): hi = x rounded once, lo = 128 + (x - hi) / step rounded to nearest, 0 .. 255."""
    hi = x.double().to(TYPES[dt])
    lo = torch.round(128.0 + (x.double() - hi.double()) / split_step(hi, dt)).clamp(0, 255).to(torch.uint8)
    return hi, lo


def split_decode(hi16, lo, dt):
    return hi16.double() + (lo.double() - 128.0) * split_step(hi16, dt)


# ---- exact cases --------------------------------------------------------------------------------------------------------------------

def ints(shape, seed, amp=3):
    return torch.randint(-amp, amp + 1, tuple(shape), generator=_g(seed)).double()


def eighths(shape, seed, amp=4):
    return torch.randint(-8 * amp, 8 * amp + 1, tuple(shape), generator=_g(seed)).double() / 8.0


def _hash_distinct(x, seed=12345):
    """True if the rows of x [R, C] (multiples of 1/16, |x| < 2^24) are pairwise distinct: an int64 random projection separates them
    (distinct hashes prove distinct rows; a collision of distinct rows fails the case, which then moves to another seed)."""
    if x.shape[0] <= 1:
        return True
    xi = torch.round(x * 16.0).to(torch.int64)
    wgt = torch.randint(1, 1 << 20, (x.shape[1],), generator=_g(seed), dtype=torch.int64)
    h = (xi * wgt[None, :]).sum(1)
    return int(torch.unique(h).numel()) == x.shape[0]


def placement_properties(ref):
    """ref [Z, M, N]: rows pairwise distinct, columns pairwise distinct, columns n / n + 4 differ in every 16-row block, slots differ."""
    Z, M, N = ref.shape
    rows = all(_hash_distinct(ref[z]) for z in range(Z))
    cols = all(_hash_distinct(ref[z].T.contiguous()) for z in range(Z))
    quads = True
    if N > 4:
        d = ref[..., :-4] != ref[..., 4:]
        pad = round_up(M, ROW_BLOCK) - M
        if pad:
            d = torch.cat([d, d[:, -1:].expand(Z, pad, N - 4)], 1)          # a partial last block is judged on the rows it has
        quads = bool(d.reshape(Z, -1, ROW_BLOCK, N - 4).any(2).all())
    slots = all(not torch.equal(ref[z], ref[z + 1]) for z in range(Z - 1))
    return {"rows": rows, "cols": cols, "quads": quads, "slots": slots}


def can_be_distinct(M, N, K, extra):
    """7^K operand rows exist: with K = 1 and nothing but a bias, more than 7 output rows cannot differ."""
    return extra or 7 ** min(K, 12) >= max(M, N)


@functools.lru_cache(maxsize=2)
def exact_case(M, N, K, batch=1, seed=0, outs=("f32",), amp_a=3, residual=True, ln=False, int_epi=False, limit=float(1 << 21)):
    """Operands, epilogue operands and expected results of one exact case (all float64 holding exactly representable values):
    a [Z, M, K], w [N, K], bias [N], residual [Z, M, N] (None if not residual), stats [M, 2] + csum [N] (ln), and `ref`: a dict of the
    expected float32 results by epilogue name -- 'plain', 'bias', 'res' (bias + residual), 'ln' / 'ln_bias'; expected(case, name, out)
    rounds one of them once to an output type.  The placement properties hold for every type in `outs` after that rounding.
    int_epi: bias and residual are integers (the split stream's lo == 128 cases).  limit: bound on |value| before the output rounding."""
    for attempt in range(64):
        s = seed * 1000 + attempt * 7919 + M * 3 + N * 5 + K * 11
        a, w = ints((batch, M, K), s + 1, amp_a), ints((N, K), s + 2)
        lone = M % ROW_BLOCK == 1 and N > 4
        if lone:
            # A last row block of ONE row cannot rely on chance for "columns n and n + 4 differ" over hundreds of column pairs: that row is
            # amp_a e_k0 and column k0 of w is +3 / -3 by the parity of n / 4, so the row's products are +-3 amp_a, alternating per quad --
            # 6 amp_a apart, more than the bias and the residual can bridge (2 + 2 apart at most; integers of at most 1 with amp_a = 1).
            k0 = K // 2
            w[:, k0] = 3.0 * (1 - 2 * ((torch.arange(N) // 4) % 2)).double()
            a[:, M - 1, :] = 0
            a[:, M - 1, k0] = float(amp_a)
        acc = product(a, w)
        bias = ints((N,), s + 3, 1) if int_epi else eighths((N,), s + 3, 1)
        res = (ints((batch, M, N), s + 4, 1) if int_epi else eighths((batch, M, N), s + 4, 1)) if residual else None
        ref = {"plain": acc, "bias": epilogue(acc, bias=bias)}
        if residual:
            ref["res"] = epilogue(acc, bias=bias, residual=res)
        stats = csum = None
        if ln:
            mean = ints((M,), s + 5, 4)
            rstd = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (M,), generator=_g(s + 6))]
            if lone:
                mean[M - 1], rstd[M - 1] = 0.0, 1.0
            stats, csum = torch.stack([mean, rstd], 1), ints((N,), s + 7, 8)
            ref["ln"] = epilogue(acc, stats=stats, csum=csum)
            ref["ln_bias"] = epilogue(acc, stats=stats, csum=csum, bias=bias)
        if max(float(v.abs().max()) for v in ref.values()) >= limit:
            continue
        if all(all(placement_properties(round_T(v, o)).values()) for v in ref.values() for o in outs):
            return {"M": M, "N": N, "K": K, "batch": batch, "a": a, "w": w, "bias": bias, "residual": res, "stats": stats, "csum": csum,
                    "ref": ref, "outs": outs, "attempt": attempt}
    raise AssertionError(f"no exact case with the placement properties for M={M} N={N} K={K} batch={batch} outs={outs}")


def expected(case, name, out):
    """The expected result of epilogue `name`, rounded once to the output type."""
    assert out in case["outs"], (out, case["outs"])
    return round_T(case["ref"][name], out)


def exact_bounds(case):
    """The magnitudes the exactness argument needs: every operand an integer of at most 3, every partial sum therefore at most 9 K <
    2^24, every expected value below 2^21 in multiples of 1/16."""
    a, w = case["a"], case["w"]
    ok = bool((a == a.round()).all()) and bool((w == w.round()).all()) and float(a.abs().max()) <= 3 and float(w.abs().max()) <= 3
    ok = ok and 9 * case["K"] < (1 << 24)
    for v in case["ref"].values():
        ok = ok and float(v.abs().max()) < (1 << 21) and bool((v * 16 == (v * 16).round()).all())
    return ok


def f32_product_in_order(a, w, reverse=False):
    """sum_k a[m][k] w[n][k] accumulated in float32 one k at a time, forward or reversed."""
    a32, w32 = a.float(), w.float()
    acc = torch.zeros(a.shape[:-1] + (w.shape[0],), dtype=torch.float32)
    ks = range(a.shape[-1] - 1, -1, -1) if reverse else range(a.shape[-1])
    for k in ks:
        acc += a32[..., k].unsqueeze(-1) * w32[:, k]
    return acc


# ---- Gaussian cases -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def gauss_case(M, N, K, batch=1, dt="f32", seed=0):
    """a, w rounded to the operand type (as float64), bias, residual, LayerNorm-consumer operands, and the product in float64 and float32."""
    s = seed * 1000 + M * 3 + N * 5 + K * 11 + 77
    T = TYPES[dt]
    a = torch.randn(batch, M, K, generator=_g(s + 1)).to(T)
    w = (torch.randn(N, K, generator=_g(s + 2)) * K ** -0.5).to(T)
    bias = torch.randn(N, generator=_g(s + 3)) * 0.5
    res = torch.randn(batch, M, N, generator=_g(s + 4))
    mean = torch.randn(M, generator=_g(s + 5)) * 0.1
    rstd = 0.5 + torch.rand(M, generator=_g(s + 6))
    csum = torch.randn(N, generator=_g(s + 7))
    return {"M": M, "N": N, "K": K, "batch": batch, "a": a, "w": w, "bias": bias, "residual": res, "stats": torch.stack([mean, rstd], 1).contiguous(),
            "csum": csum, "acc64": product(a, w), "acc32": product(a, w, torch.float32)}


def e32(r32, r64):
    return float((r32.double() - r64).abs().max())


def gauss_ref(case, **epi):
    """(float64 restatement, E32) of one epilogue on a Gaussian case."""
    r64 = epilogue(case["acc64"], **{k: (v.double() if torch.is_tensor(v) else v) for k, v in epi.items()})
    r32 = epilogue(case["acc32"], **{k: (v.float() if torch.is_tensor(v) else v) for k, v in epi.items()})
    return r64, e32(r32, r64)


# ---- the cases of the suite (tests/test_gpu_gemm_kernels.py runs them, tests/test_host_gemm_kernels.py proves their properties) ------

MN_SMALL = ((1, 1), (127, 129), (128, 128), (200, 136))
F32_K = (32, 64, 96)
TRANS_K = (1, 31, 33, 77)
S16_K = (64, 128, 192)
BIG_SHAPE, BIG_K = (513, 300, 57), (64, 128, 192, 256)
PP_SHAPE, PP_K = (529, 576), (64, 128, 192, 256, 384)
ORDER_SHAPE, ORDER_K = (8465, 1344), (64, 256, 1024)
SPLIT_SHAPE, SPLIT_K = (529, 320, 32), (64, 256)
SPLITK_NT = ((80, 128, 256, 2), (80, 128, 512, 4), (80, 128, 1024, 8), (80, 128, 2048, 16), (1409, 1921, 1024, 4))   # M, N, K, S
SPLITK_T = ((80, 128, 257, 2), (80, 128, 513, 4))
ALL16 = ("f32", "bf16", "f16")


def trans_shapes(K):
    """(rows of A, rows of W) of the transposed forms: la_gemm_ex has a bias and no residual, so K = 1 (7 possible rows) goes with 4 rows."""
    return ((4, 4),) if K == 1 else ((4, 132), (132, 4), (132, 132))


def exact_cases():
    """name -> keyword arguments of exact_case, for every exact case the GPU suite runs."""
    c = {}
    for M, N in MN_SMALL:
        for K in F32_K:
            c[f"f32nt_{M}x{N}x{K}"] = dict(M=M, N=N, K=K)
    for K in TRANS_K:
        for M, N in trans_shapes(K):
            c[f"trans_{M}x{N}x{K}"] = dict(M=M, N=N, K=K, residual=False)
    for M, N, K, _ in SPLITK_NT:
        c[f"splitk_{M}x{N}x{K}"] = dict(M=M, N=N, K=K)
    for M, N, K, _ in SPLITK_T:
        c[f"splitk_t_{M}x{N}x{K}"] = dict(M=M, N=N, K=K, residual=False)
    for M, N in MN_SMALL + ((200, 38),):
        for K in S16_K:
            c[f"s16_{M}x{N}x{K}"] = dict(M=M, N=N, K=K, outs=ALL16)
    for K in BIG_K:
        c[f"big_{K}"] = dict(M=BIG_SHAPE[0], N=BIG_SHAPE[1], K=K, batch=BIG_SHAPE[2], outs=("f32", "bf16"))
    for K in PP_K:
        c[f"pp_{K}"] = dict(M=PP_SHAPE[0], N=PP_SHAPE[1], K=K, outs=ALL16, ln=True)
    for K in ORDER_K:
        c[f"order_{K}"] = dict(M=ORDER_SHAPE[0], N=ORDER_SHAPE[1], K=K, outs=("f32", "bf16"), residual=False, ln=True)
    for K in SPLIT_K:
        c[f"split_{K}"] = dict(M=SPLIT_SHAPE[0], N=SPLIT_SHAPE[1], K=K, batch=SPLIT_SHAPE[2], outs=ALL16, amp_a=1, int_epi=True, limit=257.0)
    c["edge_200x136x64"] = dict(M=200, N=136, K=64, batch=2, outs=ALL16)
    c["edge_pp_529x576x64"] = dict(M=PP_SHAPE[0], N=PP_SHAPE[1], K=64, batch=2, outs=ALL16)
    return c
