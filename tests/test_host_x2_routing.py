"""Which kernel takes a product (DESIGN.md "Product routing"): the library's exported queries, the Python policy on top of them and the
product entries' host-side refusals -- all before any device call, without a GPU."""
import itertools

import pytest

# (M, N, K) -> f32x2.slots_for(M, N), f32x2.eligible(M, N, K), f32x2.padded_k(M, N, K), engine._x2_domain(M, N, K) as recorded from the commit
# before the rule moved into the library (the arithmetic then stood in f32x2.py and engine.py).  Edges: 188 and 192 tiles, N = 128 | 129,
# K = 255 | 256 | 384, slots beyond K's reach and beyond 16, padding of K to whole 128-element chunks per slot.
RECORDED = [
    (12000, 1024, 1024, 2, True, 1024, False),
    (12288, 1024, 1024, 1, True, 1024, True),
    (48000, 128, 1024, 2, False, 1024, False),
    (48000, 129, 1024, 2, True, 1024, False),
    (48000, 1024, 255, 1, False, 256, False),
    (48000, 1024, 256, 1, True, 256, True),
    (48000, 1024, 384, 1, True, 384, True),
    (1500, 1024, 1024, 8, False, 1024, False),
    (3000, 1024, 4096, 4, True, 4096, False),
    (48000, 3072, 1024, 1, True, 1024, True),
    (48000, 4096, 1024, 1, True, 1024, True),
    (48000, 1024, 4096, 1, True, 4096, True),
    (1024, 1024, 48000, 12, True, 49152, False),
    (24000, 320, 320, 2, False, 512, False),
    (300, 1024, 1024, 24, False, 3072, False),
    (1500, 3072, 1024, 3, True, 1152, False),
    (12000, 1024, 256, 2, False, 256, False),
    (3000, 1024, 2048, 4, True, 2048, False),
    (100, 200, 100000, 192, False, 122880, False),
]


def _tiles(M, N):
    return -(-M // 256) * -(-N // 256)


@pytest.mark.parametrize("M,N,K,slots,eligible,padded,domain", RECORDED)
def test_python_routing_answers_are_the_recorded_ones(M, N, K, slots, eligible, padded, domain):
    from lyricalignment_amd import engine, f32x2
    assert f32x2.ENABLED
    assert f32x2.slots_for(M, N) == slots
    assert f32x2.eligible(M, N, K) is eligible
    assert f32x2.padded_k(M, N, K) == padded
    assert engine._x2_domain(M, N, K) is domain


def test_exported_queries_equal_the_arithmetic_written_out():
    from lyricalignment_amd import _lib
    L = _lib.lib()
    Ms = (1, 255, 256, 257, 1500, 3000, 11776, 12000, 12032, 12033, 12288, 24000, 48000)
    Ns = (1, 127, 128, 129, 256, 257, 1024, 1025, 3072)
    Ks = (32, 128, 255, 256, 257, 384, 400, 512, 768, 1024, 4096)
    for M, N in itertools.product(Ms, Ns):
        tiles = _tiles(M, N)
        assert L.la_gemm_f16x2_slots(M, N) == max(1, -(-192 // tiles)), (M, N)
        for batch in (1, 2, 8, 32):
            assert L.la_gemm_fills_chip(M, N, batch) == int(N > 128 and tiles * batch >= 192), (M, N, batch)
        for K, slots in itertools.product(Ks, (1, 2, 3, 4, 16)):
            want = K % slots == 0 and (K // slots) % 128 == 0 and K // slots >= 256 and N > 128 and tiles * slots >= 192
            assert L.la_gemm_f16x2_domain(M, N, K, slots) == int(want), (M, N, K, slots)
    assert L.la_gemm_f16x2_domain(48000, 1024, 1024, 0) == 0
    # the two named edges: 47 x 4 = 188 tiles, 48 x 4 = 192
    assert (_tiles(12000, 1024), _tiles(12288, 1024)) == (188, 192)
    assert L.la_gemm_f16x2_domain(12000, 1024, 1024, 1) == 0 and L.la_gemm_f16x2_domain(12288, 1024, 1024, 1) == 1
    assert L.la_gemm_f16x2_slots(1500, 1024) == 8


def test_product_entries_refuse_out_of_domain_shapes_with_their_texts():
    from lyricalignment_amd import _lib
    L = _lib.lib()
    p = 4096                                       # (stand-in pointer, never dereferenced: every call below is refused before a launch)
    assert L.la_gemm_f16x2(12000, 1024, 1024, 1, p, p, p, p, p, 1024, 0, 0, 0, 0, 0) == _lib.LA_EUNSUPPORTED
    assert _lib.last_error().endswith("gemm_f16x2: M=12000 N=1024 K=1024 slots=1 outside the 256x256 kernel's domain (K / slots a multiple of 128 "
                                      "and >= 256, N > 128, >= 192 tiles x slots)")
    assert L.la_gemm_f16x2(48000, 1024, 1024, 0, p, p, p, p, p, 1024, 0, 0, 0, 0, 0) == _lib.LA_EINVAL          # no "choose" for this entry
    assert _lib.last_error().endswith("gemm_f16x2: bad sizes")
    assert L.la_gemm_f16x2_small(16, 16, 48, 1, p, p, p, p, p, 16, 0, 0, 0, 0, 0) == _lib.LA_EUNSUPPORTED
    assert _lib.last_error().endswith("gemm_f16x2_small: M=16 N=16 K=48 slots=1 outside the 128x128 kernel's domain (K / slots a multiple of 32, "
                                      "at most 64 slots)")
    assert L.la_gemm_f16x2_small(16, 16, 256, 3, p, p, p, p, p, 16, 0, 0, 0, 0, 0) == _lib.LA_EUNSUPPORTED
    assert _lib.last_error().endswith("gemm_f16x2_small: M=16 N=16 K=256 slots=3 outside the 128x128 kernel's domain (K / slots a multiple of 32, "
                                      "at most 64 slots)")
    assert L.la_gemm_f16x2_small(16, 16, 48, 0, p, p, p, p, p, 16, 0, 0, 0, 0, 0) == _lib.LA_EUNSUPPORTED       # slots = 0: chosen (1), then refused
    assert "slots=1" in _lib.last_error()
    assert L.la_gemm_f16x2_small(16, 16, 64, 1, p, p, p, p, p, 15, 0, 0, 0, 0, 0) == _lib.LA_EINVAL             # this entry's own pitch check
    assert _lib.last_error().endswith("gemm_f16x2_small: row pitches must cover N")


@pytest.mark.parametrize("name,shape", [("gemm_f16x2", (48000, 1024, 1024)), ("gemm_f16x2_small", (16, 16, 64))])
def test_product_entries_share_their_argument_checks(name, shape):
    from lyricalignment_amd import _lib
    fn = getattr(_lib.lib(), "la_" + name)
    p = 4096
    M, N, K = shape
    for nulled in range(5):                        # A, sa, W, sw, C
        ptrs = [p] * 5
        ptrs[nulled] = 0
        assert fn(M, N, K, 1, *ptrs, N, 0, 0, 0, 0, 0) == _lib.LA_EINVAL
        assert _lib.last_error().endswith(f"{name}: null pointer")
    assert fn(M, N, K, 1, p, p, p, p, p, N, 0, 0, 0, 1 << 3, 0) == _lib.LA_EINVAL
    assert _lib.last_error().endswith(f"{name}: epilogue takes BIAS, GELU, RESIDUAL, RES_GELU_GRAD only")
    assert fn(M, N, K, 1, p, p, p, p, p, N, 0, p, N, _lib.EPI_RES_GELU_GRAD, 0) == _lib.LA_EINVAL
    assert _lib.last_error().endswith(f"{name}: RES_GELU_GRAD reads the residual operand (set RESIDUAL too)")
    assert fn(M, N, K, 1, p, p, p, p, p, N, 0, 0, 0, _lib.EPI_BIAS, 0) == _lib.LA_EINVAL
    assert _lib.last_error().endswith(f"{name}: bias epilogue without pointer")
    assert fn(M, N, K, 1, p, p, p, p, p, N, 0, 0, 0, _lib.EPI_RESIDUAL, 0) == _lib.LA_EINVAL
    assert _lib.last_error().endswith(f"{name}: residual epilogue without pointer")
    assert fn(M, N, K, 1, p + 8, p, p, p, p, N, 0, 0, 0, 0, 0) == _lib.LA_EINVAL
    assert _lib.last_error().endswith(f"{name}: planes must be 16-byte aligned")
    assert fn(M, N, 0, 1, p, p, p, p, p, N, 0, 0, 0, 0, 0) == _lib.LA_EINVAL
    assert _lib.last_error().endswith(f"{name}: bad sizes")
    assert fn(0, N, K, 1, 0, 0, 0, 0, 0, N, 0, 0, 0, 0, 0) == _lib.LA_OK                                        # nothing to do


def test_python_products_validate_out_alike():
    import torch
    from lyricalignment_amd import f32x2
    a = f32x2.Planes(torch.zeros((4, 2, 64), dtype=torch.float16), torch.ones(4), 4, 64, 64)
    w = f32x2.Planes(torch.zeros((8, 2, 64), dtype=torch.float16), torch.ones(8), 8, 64, 64)
    w96 = f32x2.Planes(torch.zeros((8, 2, 96), dtype=torch.float16), torch.ones(8), 8, 96, 96)
    for fn in (f32x2.gemm, f32x2.gemm_small):
        with pytest.raises(ValueError, match="plane lengths"):
            fn(a, w96)
        with pytest.raises(ValueError, match="float32"):
            fn(a, w, out=torch.empty((4, 8), dtype=torch.float16))
        with pytest.raises(ValueError, match="float32"):
            fn(a, w, out=torch.empty((4, 9), dtype=torch.float32))
        with pytest.raises(ValueError, match="residual operand"):
            fn(a, w, residual=torch.zeros((4, 8)), gelu_grad_of=torch.zeros((4, 8)))


def test_python_encoder_route_follows_the_c_route_at_widths_off_128():
    """la_encoder_forward's encoder_x2 takes the f16x2 route without option x2_small only where K = d suits the 256 x 256 kernel; the Python
    op-by-op sequence asks the same question (it used to look at the tile count alone)."""
    from lyricalignment_amd import _lib, engine
    M = 17 * 1500
    assert _tiles(M, 320) >= 192                   # 17 clips fill the chip at d = 320 ...
    assert _lib.get_option("x2_small") == 0
    assert engine._x2_route(M, 320, 320) is False  # ... but 320 is no multiple of 128: the 256 x 256 kernel does not take it
    assert engine._x2_route(M, 384, 384) is True
    assert engine._x2_route(16 * 1500, 384, 384) is False
    with _lib.option("x2_small", 1):
        assert engine._x2_route(M, 320, 320) is True
        assert engine._x2_route(1500, 1024, 1024) is True
        assert engine._x2_route(1500, 336, 336) is False       # not a multiple of 32
