"""The GEMM reference (tests/gemm_reference.py) proved on the CPU, and every host-side rejection of la_gemm, la_gemm_ex, la_gemm_fused_ln,
la_gemm_split and la_ln_stats_finalize through the C ABI.  Runs without a GPU: the rejected calls carry stand-in pointers and must come
back with their status before any launch.

Per exact case the GPU suite runs (gemm_reference.exact_cases): the magnitude bounds of the exactness argument; a float32 product
accumulated one k at a time in forward and in reversed order equals the int64 product (on all rows, or on 64 evenly spaced rows of every
slot where the case has more than 2^21 outputs: the loop is K passes over the output); the expected result of every epilogue in every
output type has pairwise distinct rows and columns, columns n and n + 4 that differ in every 16-row block, and batch slots that differ.
The restated routing arithmetic (split-K planner, tile order, la_gemm_fills_chip) is checked against the figures the suite relies on.

Two LA_CHECK_ARGs of gemm_run_ldw cannot be reached through the C ABI and are not listed: "no LayerNorm fold with transposed operands"
(transposed operands are float32, which la_gemm_fused_ln refuses first) and "row statistics without the column sums" (without column sums
the call has either no second output -- refused first -- or both roles)."""
import ctypes

import pytest
import torch

import gemm_reference as G

A0, W0, C0, C1, X0, X1, X2 = (0x10000000 * i for i in range(1, 8))        # stand-ins: non-null, 256-byte aligned, far apart, never dereferenced
CASES = G.exact_cases()


def _lib():
    from lyricalignment_amd import _lib
    return _lib


# ---- the reference ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_case_is_exact_in_any_order_and_pins_every_placement(name):
    case = G.exact_case(**CASES[name])
    assert G.exact_bounds(case)
    a, w = case["a"], case["w"]
    Z, M, K = a.shape
    if Z * M * w.shape[0] > (1 << 21):
        a = a[:, torch.linspace(0, M - 1, 64).round().long()]
    want = G.product_int64(a, w)
    assert int(want.abs().max()) < (1 << 24)
    for reverse in (False, True):
        assert torch.equal(G.f32_product_in_order(a, w, reverse).to(torch.int64), want), ("reversed" if reverse else "forward")
    assert torch.equal(G.product(a, w).to(torch.int64), want)
    for epi, ref in case["ref"].items():
        for out in case["outs"]:
            props = G.placement_properties(G.round_T(ref, out))
            assert all(props.values()), (name, epi, out, props)
    if "limit" in CASES[name]:
        assert max(float(v.abs().max()) for v in case["ref"].values()) <= 256       # an integer of at most 2^8 is a bf16 / f16 value


def test_a_generator_that_cannot_meet_the_properties_says_so():
    assert not G.can_be_distinct(132, 4, 1, extra=False) and G.can_be_distinct(4, 4, 1, extra=False) and G.can_be_distinct(132, 132, 31, extra=False)
    with pytest.raises(AssertionError):
        G.exact_case(132, 4, 1, residual=False)
    props = G.placement_properties(torch.zeros(1, 32, 8, dtype=torch.float64))
    assert not any(props[k] for k in ("rows", "cols", "quads"))
    x = torch.arange(32 * 8, dtype=torch.float64).reshape(1, 32, 8)
    assert all(G.placement_properties(x).values())
    x[0, 16:, 4:] = x[0, 16:, :4]                                                       # rows 16..31: column n + 4 repeats column n
    assert not G.placement_properties(x)["quads"]


def test_split_k_planner_and_tile_order_as_the_suite_relies_on_them():
    for M, N, K, S in G.SPLITK_NT + G.SPLITK_T:
        s, kc, tail = G.splitk_plan(M, N, K)
        assert s == S and 0 < tail <= kc and (s - 1) * kc + tail == K, (M, N, K, s, kc, tail)
    assert G.splitk_plan(80, 128, 257) == (2, 160, 97) and G.splitk_plan(80, 128, 513)[2] == 33
    assert G.splitk_plan(1409, 1921, 1024)[0] == 4 and G.cdiv(1409, 128) * G.cdiv(1921, 128) == 192       # the S = 4 rule, not the doubling
    for M, N in G.MN_SMALL:
        for K in G.F32_K:
            assert G.splitk_plan(M, N, K)[0] == 1
    M, N = G.ORDER_SHAPE
    tm, tn = G.cdiv(M, 256), G.cdiv(N, 256)
    assert (tm, tn) == (34, 6)
    assert [G.pp_group(N, K) for K in G.ORDER_K] == [(5, 32), (5, 32), (4, 32)]
    for K in G.ORDER_K:
        group, mblock = G.pp_group(N, K)
        seen = {G.tile_coord_mb(t, tm, tn, group, mblock) for t in range(tm * tn)}
        assert seen == {(i, j) for i in range(tm) for j in range(tn)}
    assert G.pp_group(G.PP_SHAPE[1], 64) == (3, 0)
    m, n, z = G.BIG_SHAPE
    assert G.cdiv(m, 256) * G.cdiv(n, 128) * z >= 512 > G.cdiv(m, 256) * G.cdiv(n, 128) * (z - 1)


def test_split_stream_encoding_round_trips():
    for dt in ("bf16", "f16"):
        x = torch.cat([torch.randn(4096, generator=G._g(5), dtype=torch.float64) * 3, torch.tensor([0.0, 1.0, -256.0, 3e-6, 255.0], dtype=torch.float64)])
        hi, lo = G.split_encode(x, dt)
        back = G.split_decode(hi, lo, dt)
        assert bool(((back - x).abs() <= 0.5 * G.split_step(hi, dt) * (1 + 1e-12)).all())
        assert bool((lo[-5:-2] == 128).all()) and torch.equal(back[-5:-2], x[-5:-2])
        from lyricalignment_amd import ops
        assert bool(((ops.split_decode(hi, lo).double() - back).abs() <= 2.0 ** -22 * back.abs()).all())      # the decoder of the package, in float32
        assert bool((G.split_step(hi, dt)[:-5] * 254 / G.ulp_T(hi.double(), dt)[:-5] - 1).abs().max() < 1e-12)


def test_segment_statistics_combine_to_the_row_statistics():
    x = torch.randn(7, 320, generator=G._g(3), dtype=torch.float64)
    st = G.stats_finalize(G.segment_stats(x), eps=1e-5)
    assert float((st[:, 0] - x.mean(1)).abs().max()) < 1e-14
    assert float((st[:, 1] - 1 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)).abs().max()) < 1e-13


# ---- host-side argument checks ------------------------------------------------------------------------------------------------------

GEMM = ("dtype", "M", "N", "K", "batch", "A", "lda", "strideA", "W", "C", "ldc", "strideC", "bias", "residual", "ldr", "strideR", "epilogue", "stream")
GEMM_EX = ("dtype", "M", "N", "K", "batch", "A", "lda", "strideA", "W", "ldw", "strideW", "C", "ldc", "strideC", "bias", "epilogue", "stream")
FUSED = GEMM[:-1] + ("C2", "ldc2", "strideC2", "ln_stats", "ln_csum", "ln_part", "stream")
SPLIT = ("dtype", "M", "N", "K", "batch", "A", "lda", "strideA", "W", "hi", "lo", "ld", "stride", "bias", "residual", "ldr", "strideR", "epilogue",
         "ln_part", "stream")
ENTRY = {"gemm": ("la_gemm", GEMM), "ex": ("la_gemm_ex", GEMM_EX), "fused": ("la_gemm_fused_ln", FUSED), "split": ("la_gemm_split", SPLIT)}
FILL = dict(dtype=1, M=4096, N=3072, ldc=3072, ld=3072, ldc2=3072)              # 16 x 12 = 192 tiles of 256 x 256: fills the chip


def _args(**kw):
    a = dict(dtype=0, M=64, N=64, K=64, batch=1, A=A0, lda=64, strideA=0, W=W0, ldw=64, strideW=0, C=C0, ldc=64, strideC=0, bias=0, residual=0,
             ldr=0, strideR=0, epilogue=0, stream=0, C2=0, ldc2=0, strideC2=0, ln_stats=0, ln_csum=0, ln_part=0, hi=C0, lo=C1, ld=64, stride=0)
    a.update(kw)
    return a


def _call(entry, **kw):
    lib = _lib()
    name, order = ENTRY[entry]
    a = _args(**kw)
    return getattr(lib.lib(), name)(*[a[k] for k in order]), lib.last_error()


def _rejected(entry, status, message, **kw):
    rc, err = _call(entry, **kw)
    assert rc == status and message in err, (entry, kw, rc, err)


GEMM_BAD = [
    (dict(A=0), "null pointer"), (dict(W=0), "null pointer"), (dict(C=0), "null pointer"),
    (dict(K=0), "bad sizes"), (dict(K=-32), "bad sizes"), (dict(M=-1), "bad sizes"), (dict(N=-5), "bad sizes"), (dict(batch=-1), "bad sizes"),
    (dict(dtype=3), "bad dtype"), (dict(dtype=-1), "bad dtype"),
    (dict(K=48), "must be a multiple of 32"), (dict(dtype=1, K=32), "must be a multiple of 64"), (dict(dtype=2, K=96), "must be a multiple of 64"),
    (dict(lda=66), "16-byte aligned"), (dict(strideA=2), "16-byte aligned"), (dict(A=A0 + 4), "16-byte aligned"), (dict(W=W0 + 8), "16-byte aligned"),
    (dict(dtype=1, lda=68), "16-byte aligned"),
    (dict(epilogue=G.EPI_RESIDUAL), "residual epilogue without pointer"), (dict(epilogue=G.EPI_BIAS), "bias epilogue without pointer"),
    (dict(dtype=1, epilogue=G.TRANS_A), "float32 only"), (dict(dtype=2, epilogue=G.TRANS_W), "float32 only"),
]


@pytest.mark.parametrize("entry", ["gemm", "ex"])
def test_gemm_rejects_bad_arguments_on_the_host(entry):
    lib = _lib()
    for change, message in GEMM_BAD:
        if entry == "ex" and "residual" in message:
            continue                                            # la_gemm_ex has no residual
        _rejected(entry, lib.LA_EINVAL, message, **{"ldw": max(64, change.get("K", 64)), **change})


def test_gemm_ex_rejects_bad_layouts_on_the_host():
    E = _lib().LA_EINVAL
    TA, TW = G.TRANS_A, G.TRANS_W
    _rejected("ex", E, "ldw smaller than a row of W", ldw=32)
    _rejected("ex", E, "ldw smaller than a row of W", ldw=32, N=64, K=16, epilogue=TW)
    _rejected("ex", E, "ldw smaller than a row of W", ldw=0)
    for change in (dict(M=66, lda=68, epilogue=TA), dict(lda=60, epilogue=TA), dict(N=66, ldw=68, epilogue=TW), dict(M=62, epilogue=TA | TW)):
        _rejected("ex", E, "needs rows % 4 == 0 and a pitch >= rows", **change)
    _rejected("ex", E, "must be a multiple of 32", K=33, ldw=64)                          # no transposed operand: K % 32
    _rejected("ex", E, "pitched to the rounded-up K", K=33, ldw=40, epilogue=TA)          # W is K-contiguous: ldw >= 64
    _rejected("ex", E, "pitched to the rounded-up K", K=33, lda=40, epilogue=TW)          # A is K-contiguous: lda >= 64
    _rejected("ex", E, "W batch stride / row pitch", ldw=66)
    _rejected("ex", E, "W batch stride / row pitch", strideW=6)
    # what the same layouts accept gets as far as the last check, the bias flag without its pointer
    for change in (dict(K=33, ldw=64, epilogue=TA), dict(K=33, lda=64, epilogue=TW), dict(K=33, epilogue=TA | TW), dict(K=1, epilogue=TA | TW)):
        change["epilogue"] |= G.EPI_BIAS
        _rejected("ex", E, "bias epilogue without pointer", **change)


def test_fused_ln_rejects_on_the_host():
    lib = _lib()
    E, U = lib.LA_EINVAL, lib.LA_EUNSUPPORTED
    _rejected("fused", U, "16-bit compute dtypes only", C2=X0)
    _rejected("fused", U, "16-bit compute dtypes only", dtype=3, C2=X0)
    _rejected("fused", E, "neither a second output nor", dtype=1)
    _rejected("fused", E, "neither a second output nor", dtype=2, ln_stats=X1)
    f32out = G.EPI_OUT_F32
    _rejected("fused", U, "does not run on the 256x256 kernel", dtype=1, C2=X0, epilogue=f32out)                     # one tile
    _rejected("fused", U, "does not run on the 256x256 kernel", **{**FILL, "M": 4096 - 256}, C2=X0, epilogue=f32out)  # 180 tiles
    _rejected("fused", U, "does not run on the 256x256 kernel", **{**FILL, "N": 128, "M": 1 << 20}, C2=X0, epilogue=f32out)
    _rejected("fused", U, "does not run on the 256x256 kernel", **FILL, C2=X0, epilogue=f32out | G.EPI_MISH)
    with lib.option("gemm_tile", 128):
        _rejected("fused", U, "does not run on the 256x256 kernel", **FILL, C2=X0, epilogue=f32out)
    copy = "the 16-bit copy accompanies an f32 result"
    _rejected("fused", E, copy, **FILL, C2=X0)                                                   # 16-bit result
    _rejected("fused", E, copy, **{**FILL, "ldc2": 3076}, C2=X0, epilogue=f32out)
    _rejected("fused", E, copy, **FILL, C2=X0, strideC2=8, epilogue=f32out)
    _rejected("fused", E, copy, **{**FILL, "ldc": 3074, "ldc2": 3074}, C2=X0, epilogue=f32out)
    _rejected("fused", E, copy, **FILL, C2=X0 + 4, epilogue=f32out)
    _rejected("fused", E, "not both", **FILL, C2=X0, ln_stats=X1, epilogue=f32out)
    _rejected("fused", E, "not both", **FILL, C2=X0, ln_csum=X2, epilogue=f32out)
    _rejected("fused", E, "takes batch 1", **FILL, batch=2, ln_stats=X1, ln_csum=X2)
    part = "partial statistics go with the 16-bit copy"
    _rejected("fused", E, part, **FILL, ln_stats=X1, ln_csum=X2, ln_part=X0)
    _rejected("fused", E, part, **{**FILL, "N": 3080, "ldc": 3080, "ldc2": 3080}, C2=X0, ln_part=X1, epilogue=f32out)
    _rejected("fused", E, part, **FILL, batch=2, C2=X0, ln_part=X1, epilogue=f32out)
    _rejected("fused", E, part, **FILL, C2=X0, ln_part=X1 + 4, epilogue=f32out)
    # the checks of the plain entry come first
    _rejected("fused", E, "null pointer", **FILL, C=0, C2=X0)
    _rejected("fused", E, "must be a multiple of 64", **FILL, K=96, C2=X0)
    if not lib.has_experiments():
        _rejected("fused", U, "in-loop row statistics", **FILL, ln_csum=X2)


def test_gemm_split_rejects_on_the_host():
    lib = _lib()
    E, U = lib.LA_EINVAL, lib.LA_EUNSUPPORTED
    _rejected("split", U, "16-bit compute dtypes only", **{**FILL, "dtype": 0})
    for ptr in ("A", "W", "hi", "lo"):
        _rejected("split", E, "null pointer", **FILL, **{ptr: 0})
    _rejected("split", E, "bad sizes", **FILL, K=0)
    _rejected("split", E, "bad sizes", **FILL, batch=-1)
    shape = "does not run on the 256x256 kernel the split epilogue is built into"
    _rejected("split", U, shape, dtype=1)
    _rejected("split", U, shape, **{**FILL, "M": 4096 - 256})
    _rejected("split", U, shape, **{**FILL, "N": 128, "M": 1 << 20})
    _rejected("split", U, shape, **FILL, K=96)
    _rejected("split", U, shape, **FILL, K=32)
    for bits in (G.EPI_MISH, G.EPI_OUT_F32, G.EPI_GELU_ERF, G.TRANS_A):
        _rejected("split", E, "epilogue takes BIAS, GELU, RESIDUAL only", **FILL, epilogue=bits)
    for change in (dict(lda=68), dict(strideA=4), dict(A=A0 + 8), dict(W=W0 + 2)):
        _rejected("split", E, "16-byte aligned", **FILL, **change)
    _rejected("split", E, "bias epilogue without pointer", **FILL, epilogue=G.EPI_BIAS)
    _rejected("split", E, "row pitch below N", **{**FILL, "ld": 3071})
    _rejected("split", E, "row pitch below N", **FILL, hi=C0 + 1)
    part = "partial statistics need N % 64 == 0, batch 1"
    _rejected("split", E, part, **{**FILL, "N": 3080, "ld": 3080}, ln_part=X0)
    _rejected("split", E, part, **FILL, batch=2, stride=4096 * 3072, ln_part=X0)
    _rejected("split", E, part, **FILL, ln_part=X0 + 4)
    overlap = "must not overlap the (hi, lo) stream"
    _rejected("split", E, overlap, **FILL, hi=A0)
    _rejected("split", E, overlap, **FILL, lo=A0 + 64 * 2 * 4095)                 # the last row of A
    _rejected("split", E, overlap, **FILL, hi=W0 - 2 * (4095 * 3072 + 3072) + 16)    # the stream's last bytes reach into W
    _rejected("split", E, overlap, **FILL, lo=W0 + 3072 * 64 * 2 - 16)


def test_ln_stats_finalize_rejects_on_the_host():
    lib = _lib()
    L = lib.lib()
    for part, slots, M, stats in ((0, 5, 7, X1), (X0, 0, 7, X1), (X0, -1, 7, X1), (X0, 5, -7, X1), (X0, 5, 7, 0)):
        assert L.la_ln_stats_finalize(part, slots, M, 1e-5, stats, 0) == lib.LA_EINVAL and "ln_stats_finalize: bad arguments" in lib.last_error()
    assert L.la_ln_stats_finalize(0, 0, 0, 1e-5, 0, 0) == lib.LA_OK


def test_zero_size_calls_return_before_any_pointer_is_looked_at():
    lib = _lib()
    nothing = dict(A=0, W=0, C=0, hi=0, lo=0)
    for empty in (dict(M=0), dict(N=0), dict(batch=0)):
        for entry, more in (("gemm", {}), ("ex", {}), ("fused", dict(dtype=1, C2=X0)), ("split", dict(dtype=1))):
            rc, err = _call(entry, **nothing, **empty, **more)
            assert rc == lib.LA_OK, (entry, empty, err)


def test_fills_chip_at_its_boundaries():
    L = _lib().lib()
    for M, N, batch in ((256 * 191, 256, 1), (256 * 191 + 1, 256, 1), (256 * 192, 129, 1), (256 * 192, 128, 1), (1, 129, 191), (1, 129, 192),
                        (1, 128, 192), (256, 256 * 191, 1), (256, 256 * 191 + 1, 1), (257, 257, 47), (257, 257, 48), (1 << 20, 128, 64)):
        assert bool(L.la_gemm_fills_chip(M, N, batch)) == G.fills_chip(M, N, batch), (M, N, batch)
    assert [L.la_gemm_fills_chip(*s) for s in ((256 * 191, 256, 1), (256 * 191 + 1, 256, 1), (256 * 192, 128, 1), (256 * 192, 129, 1))] == [0, 1, 0, 1]
    assert L.la_gemm_fills_chip(*G.ORDER_SHAPE, 1) == 1 and L.la_gemm_fills_chip(*G.SPLIT_SHAPE) == 1 and L.la_gemm_fills_chip(*G.PP_SHAPE, 1) == 0
