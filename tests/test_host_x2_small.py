"""Option x2_small and the 128 x 128 f16x2 product's host side (include/lyricalign.h la_gemm_f16x2_small, f32x2.gemm_small): what is
checked before any launch, without a GPU."""
import pytest
import torch


def test_x2_small_option_exists_defaults_off_and_round_trips():
    from lyricalignment_amd import _lib
    assert _lib.get_option("x2_small") == 0
    with _lib.option("x2_small", 1):
        assert _lib.get_option("x2_small") == 1
    assert _lib.get_option("x2_small") == 0


def test_small_slot_rule_fills_two_workgroups_per_cu_and_keeps_256_of_k():
    from lyricalignment_amd import f32x2
    # batch-1 encoder shapes (M = 1500) and the GRU input projection (N = 6 x 384)
    assert f32x2.slots_small(1500, 3072, 1024) == 2
    assert f32x2.slots_small(1500, 1024, 1024) == 4
    assert f32x2.slots_small(1500, 4096, 1024) == 1
    assert f32x2.slots_small(1500, 1024, 4096) == 4
    assert f32x2.slots_small(1500, 2304, 1024) == 2
    for M, N, K in ((1, 1, 32), (7, 300, 384), (1500, 1024, 512), (64, 64, 4096)):
        s = f32x2.slots_small(M, N, K)
        assert s >= 1 and K % (32 * s) == 0 and (s == 1 or K // s >= 256)


def test_gemm_small_rejects_bad_operands_before_any_launch():
    from lyricalignment_amd import f32x2
    a = f32x2.Planes(torch.zeros((4, 2, 64), dtype=torch.float16), torch.ones(4), 4, 64, 64)
    w = f32x2.Planes(torch.zeros((8, 2, 96), dtype=torch.float16), torch.ones(8), 8, 96, 96)
    with pytest.raises(ValueError):
        f32x2.gemm_small(a, w)                                            # plane lengths differ
    w = f32x2.Planes(torch.zeros((8, 2, 64), dtype=torch.float16), torch.ones(8), 8, 64, 64)
    with pytest.raises(ValueError):
        f32x2.gemm_small(a, w, out=torch.empty((4, 8), dtype=torch.float16))    # not a float32 result
    with pytest.raises(ValueError):
        f32x2.gemm_small(a, w, out=torch.empty((4, 9), dtype=torch.float32))    # wrong shape


def test_entry_point_refuses_out_of_domain_arguments_on_the_host():
    from lyricalignment_amd import _lib
    L = _lib.lib()
    p = 4096                                       # (never dereferenced: every call below is refused before a launch)
    # K / slots not a multiple of 32
    assert L.la_gemm_f16x2_small(16, 16, 48, 1, p, p, p, p, p, 16, 0, 0, 0, 0, 0) == _lib.LA_EUNSUPPORTED
    assert "domain" in _lib.last_error()
    assert L.la_gemm_f16x2_small(16, 16, 256, 3, p, p, p, p, p, 16, 0, 0, 0, 0, 0) == _lib.LA_EUNSUPPORTED
    # bad epilogue bits, bias flag without pointer, null operands
    assert L.la_gemm_f16x2_small(16, 16, 64, 1, p, p, p, p, p, 16, 0, 0, 0, 1 << 3, 0) == _lib.LA_EINVAL
    assert L.la_gemm_f16x2_small(16, 16, 64, 1, p, p, p, p, p, 16, 0, 0, 0, _lib.EPI_BIAS, 0) == _lib.LA_EINVAL
    assert L.la_gemm_f16x2_small(16, 16, 64, 1, 0, p, p, p, p, 16, 0, 0, 0, 0, 0) == _lib.LA_EINVAL
