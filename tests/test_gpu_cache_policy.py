"""Cache-policy options of the encoder's hot kernels (include/lyricalign.h: cp_epi16, cp_split_st, cp_split_ld, cp_gemm_a, cp_attn_qo,
cp_attn_kv): a policy is a modifier bit of a store or load instruction -- where a line is kept, never what is written -- so every kernel's
raw output under every policy value must equal its output at policy 0 of the same build, bit for bit.  Every test leaves the options at the
values it found (the shipped defaults: cp_epi16 = 1, the others 0), whatever happens inside it.

GEMM (the 256 x 256 kernel, option gemm_tile = 512 where the shape alone would not route there): M = 300, N = 320 -- two tiles each way with
ragged edges; interior wave tiles take the 16-bit staging (cp_epi16's stores) or the split epilogue's wide passes (cp_split_st / cp_split_ld),
edge wave tiles the element-wise float32 staging, which no policy touches -- at K = 64 (the quadrant ping-pong loop, both prefetch predicates
false, then true), 256 and 384 (the hand-placed loop, whose A-operand DMA pieces cp_gemm_a marks: its tail alone, and a ring turn before
it); K = 1024 once at M = 512, N = 256.  The split-stream form runs 48 batch slots: la_gemm_split routes by shape alone and asks for 192 tiles.
Attention: 1 clip x 65 frames x 2 heads (one key in the last tile) and 1 x 257 x 8 (the pairs % 8 == 0 block order; the 256-query workgroup
from 256 frames on), the 4-wave and the 8-wave form, bfloat16, float16 and bfloat16 with exp2-domain scores (q_log2)."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

M, N = 300, 320
SPLIT_SLOTS = 48
DTYPES = (torch.bfloat16, torch.float16)
RANGES = {"cp_epi16": 2, "cp_split_st": 1, "cp_split_ld": 1, "cp_gemm_a": 1, "cp_attn_qo": 1, "cp_attn_kv": 1}
DEFAULTS = {"cp_epi16": 1, "cp_split_st": 0, "cp_split_ld": 0, "cp_gemm_a": 0, "cp_attn_qo": 0, "cp_attn_kv": 0}
GEMM_POLICIES = [{"cp_epi16": 1}, {"cp_epi16": 2}, {"cp_split_st": 1}, {"cp_split_ld": 1}, {"cp_gemm_a": 1},
                 {"cp_epi16": 1, "cp_split_st": 1, "cp_split_ld": 1, "cp_gemm_a": 1}, {"cp_epi16": 2, "cp_split_st": 1, "cp_split_ld": 1, "cp_gemm_a": 1}]
ATTN_POLICIES = [{"cp_attn_qo": 1}, {"cp_attn_kv": 1}, {"cp_attn_qo": 1, "cp_attn_kv": 1}]


@contextlib.contextmanager
def _policy(values):
    """Every policy option at 0 but the given ones; afterwards, whatever happened in between, every option is back at the value it had on
    entry (its default, which is 0 for all but cp_epi16: later tests run the library as it ships)."""
    from lyricalignment_amd import _lib
    found = {name: _lib.get_option(name) for name in RANGES}
    try:
        for name in RANGES:
            _lib.set_option(name, values.get(name, 0))
        yield
    finally:
        for name, v in found.items():
            _lib.set_option(name, v)


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _bits(t):
    return t.view(torch.uint8) if t.dtype == torch.uint8 else t.view(torch.int16)


def _gemm_forms(K, dtype, m=M, n=N, forms=("plain", "ln", "ln_gelu", "split")):
    """{form: fn() -> tuple of raw outputs}; every fn starts from the same inputs on every call."""
    from lyricalignment_amd import ops
    a = _rand(m, K, seed=11, scale=0.5).to(dtype).cuda()
    w = _rand(n, K, seed=12, scale=K ** -0.5).to(dtype).cuda()
    bias, csum = _rand(n, seed=13).cuda(), (_rand(n, seed=14) * 0.1).cuda()
    rows = torch.arange(m)
    stats = torch.stack([0.01 * (rows % 50).float(), 0.5 + 0.25 * (rows % 4).float()], dim=1).contiguous().cuda()
    out = {}
    if "plain" in forms:
        out["plain"] = lambda: (ops.gemm(a, w, bias=bias).clone(),)
    if "ln" in forms:
        out["ln"] = lambda: (ops.gemm(a, w, bias=bias, ln_stats=stats, ln_csum=csum).clone(),)
    if "ln_gelu" in forms:
        out["ln_gelu"] = lambda: (ops.gemm(a, w, bias=bias, gelu=True, ln_stats=stats, ln_csum=csum).clone(),)
    if "split" in forms:
        az = _rand(SPLIT_SLOTS * m, K, seed=15, scale=0.5).to(dtype).cuda()
        hi0 = _rand(SPLIT_SLOTS, m, n, seed=16).to(dtype).cuda()
        lo0 = torch.randint(1, 256, (SPLIT_SLOTS, m, n), generator=torch.Generator().manual_seed(17), dtype=torch.uint8).cuda()

        def split():
            hi, lo = hi0.clone(), lo0.clone()
            ops.gemm_split(az, w, hi, lo, bias=bias, in_place=True, M=m, lda=K, batch=SPLIT_SLOTS, stride_a=m * K, stride_c=m * n, ld=n)
            return hi, lo

        out["split"] = split
    return out


def _assert_same(ref, got, what):
    for r, g in zip(ref, got):
        assert r.dtype == g.dtype and r.shape == g.shape
        assert torch.equal(_bits(r), _bits(g)), what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", (64, 256, 384))
def test_gemm_outputs_do_not_depend_on_the_cache_policy(K, dtype):
    from lyricalignment_amd import _lib
    with _lib.option("gemm_tile", 512):
        forms = _gemm_forms(K, dtype)
        with _policy({}):
            ref = {name: fn() for name, fn in forms.items()}
        assert not torch.equal(_bits(ref["plain"][0]), _bits(ref["ln"][0]))          # (the forms are different launches)
        for pol in GEMM_POLICIES:
            with _policy(pol):
                for name, fn in forms.items():
                    _assert_same(ref[name], fn(), f"{name} K={K} {dtype} under {pol}")
        with _policy({}):                                                            # and policy 0 is back: the reference once more
            for name, fn in forms.items():
                _assert_same(ref[name], fn(), f"{name} K={K} {dtype} at policy 0 again")


def test_gemm_long_k_all_policies_together():
    from lyricalignment_amd import _lib
    with _lib.option("gemm_tile", 512):
        fn = _gemm_forms(1024, torch.bfloat16, m=512, n=256, forms=("plain",))["plain"]
        with _policy({}):
            ref = fn()
        for pol in GEMM_POLICIES[-2:]:
            with _policy(pol):
                _assert_same(ref, fn(), f"plain K=1024 under {pol}")


@pytest.mark.parametrize("frames,heads", ((65, 2), (257, 8)))
def test_attention_outputs_do_not_depend_on_the_cache_policy(frames, heads):
    from lyricalignment_amd import _lib, ops
    for dtype, q_log2 in ((torch.bfloat16, False), (torch.float16, False), (torch.bfloat16, True)):
        qkv = _rand(frames, 3 * heads * 64, seed=21)
        qkv[:, : heads * 64] *= 0.125 * (1.4426950408889634 if q_log2 else 1.0)
        qkv = qkv.to(dtype).cuda()
        for nw in (4, 8):
            with _lib.option("attn_nw", nw):
                with _policy({}):
                    ref = ops.attention(qkv, 1, frames, heads, q_log2=q_log2).clone()
                assert bool(torch.isfinite(ref.float()).all())
                for pol in ATTN_POLICIES:
                    with _policy(pol):
                        got = ops.attention(qkv, 1, frames, heads, q_log2=q_log2).clone()
                    _assert_same((ref,), (got,), f"attention {frames}x{heads} {dtype} q_log2={q_log2} nw={nw} under {pol}")


def test_options_round_trip_and_refuse_values_out_of_range():
    from lyricalignment_amd import _lib
    found = {name: _lib.get_option(name) for name in RANGES}
    assert found == DEFAULTS                                                         # (the measured defaults: profiles/cache_policy.txt)
    try:
        for name, top in RANGES.items():
            for v in range(top + 1):
                _lib.set_option(name, v)
                assert _lib.get_option(name) == v
            for bad in (top + 1, -1, 1 << 40):
                rc = _lib.lib().la_set_option(name.encode(), bad)
                assert rc == _lib.LA_EINVAL, (name, bad, rc)
                with pytest.raises(ValueError):
                    _lib.set_option(name, bad)
                assert _lib.get_option(name) == top                                  # a refused value changes nothing
            _lib.set_option(name, 0)
    finally:
        for name, v in found.items():
            _lib.set_option(name, v)
