"""The restatement of the emission head (tests/head_reference.py) pinned to oracle/model_oracle.py in float64 and to the reference's own
recorded output (tests/golden/emission_prep.npz), the bracket for a float32 device's silence terms checked against two float32 sigmoids on
the CPU, and every host-side rejection of la_fc_emissions / la_fc_emissions_x2 / la_emissions_from_logits and of their workspace queries
through the C ABI.  Runs without a GPU: the rejected calls carry stand-in pointers and must come back before any launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

import head_reference as H
from conftest import load_npz
from oracle import model_oracle as mo

TIGHT = 1e-12        # two float64 evaluations of the same formulas


def _labels_for(V, variant, B, Lmax, seed):
    _, hi = H.norm_range(V, variant)
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(1, hi + 1, (B, Lmax + 2), generator=g, dtype=torch.int32)
    return lab


def _compact_from_oracle(lp, ls, labels, n_labels, max_labels):
    """The oracle's full (lp [B][T][classes], ls [B][T][1]) in the compact layout, -1000 for class ids outside 1..classes."""
    B, T, C = lp.shape
    em = torch.full((B, T, 1 + max_labels), math.nan, dtype=lp.dtype)
    em[..., 0] = ls[..., 0]
    for b in range(B):
        for n in range(min(max(int(n_labels[b]), 0), max_labels)):
            c = int(labels[b, n])
            em[b, :, 1 + n] = lp[b, :, c - 1] if 1 <= c <= C else -1000.0
    return em


def _same(a, b, tol):
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    ok = ~torch.isnan(a)
    assert H.rel_err(a[ok], b[ok]) <= tol, H.rel_err(a[ok], b[ok])


@pytest.mark.parametrize("variant", [H.CTC, H.PLAIN])
@pytest.mark.parametrize("V", [3, 11, 300])
def test_restatement_matches_the_oracle_in_float64(variant, V):
    """Gaussian rows, a +1e4 offset, a spike that clamps the other classes at -1000, -inf columns, saturated silence logits; n_labels of 0,
    1, max_labels and max_labels + 3 (clamped), a repeated label and class ids 0, -1, hi + 1, V."""
    B, T, Lmax = 4, 9, 6
    g = torch.Generator().manual_seed(V)
    lg = torch.randn(B, T, V, generator=g, dtype=torch.float64) * 4
    lg[0, 1] += 1e4
    lg[1, 2, V // 2] = 3000.0
    lg[1, 3, 0] = 3000.0
    if V > 3:
        lg[2, 4, 1:V - 2] = -math.inf
    lg[2, 5, V - 1], lg[2, 6, V - 1], lg[3, 0, V - 1] = 800.0, -800.0, 17.0
    _, hi = H.norm_range(V, variant)
    labels = _labels_for(V, variant, B, Lmax, V + 1)
    labels[2, 1] = labels[2, 0]
    labels[3, :4] = torch.tensor([0, -1, hi + 1, V], dtype=torch.int32)
    n_labels = torch.tensor([0, 1, Lmax, Lmax + 3], dtype=torch.int32)
    em = H.emissions(lg, labels, n_labels, Lmax, variant)
    lp, ls = (mo.emission_prep_ctc if variant == H.CTC else mo.emission_prep_plain)(lg)
    assert lp.shape[-1] == hi
    _same(em, _compact_from_oracle(lp, ls, labels, n_labels, Lmax), TIGHT)
    w = H.written(n_labels, Lmax)
    assert torch.equal(~torch.isnan(em[:, 0]), w) and w.sum(1).tolist() == [1, 2, Lmax + 1, Lmax + 1]
    assert bool((em[3, :, 1:5] == -1000.0).all()) and torch.equal(em[2, :, 1], em[2, :, 2])
    assert bool((em[~torch.isnan(em)] >= -1000.0).all())
    if variant == H.CTC:
        assert float(em[2, 6, 0]) == -1000.0 and float(em[2, 5, 0]) == 0.0 and bool((em[2, 5, 1:] == -1000.0).all())


@pytest.mark.parametrize("variant", ["ctc", "plain"])
def test_restatement_matches_the_recorded_reference_output(variant):
    """tests/golden/emission_prep.npz holds what the reference computed in float32 (saturated silence both ways, a dominating column, a
    3000 in column 0): the restatement in float32 within 1e-5 of it, with the same entries at -1000."""
    z = load_npz("emission_prep.npz")
    lg = torch.from_numpy(z[f"{variant}/logits"])
    lp, ls = torch.from_numpy(z[f"{variant}/lp"]), torch.from_numpy(z[f"{variant}/ls"])
    var = H.CTC if variant == "ctc" else H.PLAIN
    B, T, V = lg.shape
    _, hi = H.norm_range(V, var)
    assert lp.shape == (B, T, hi) and ls.shape == (B, T, 1) and lg.dtype == torch.float32
    labels = torch.arange(1, hi + 1, dtype=torch.int32).repeat(B, 1)            # every class once, in order
    n_labels = torch.full((B,), hi, dtype=torch.int32)
    em = H.emissions(lg, labels, n_labels, hi, var)
    assert em.dtype == torch.float32 and not bool(torch.isnan(em).any())
    np.testing.assert_allclose(em[..., 0].numpy(), ls[..., 0].numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(em[..., 1:].numpy(), lp.numpy(), rtol=0, atol=1e-5)
    assert int((em[..., 1:] == -1000).sum()) == int((lp == -1000).sum()) > 0
    assert torch.equal(em[..., 0] == -1000, ls[..., 0] == -1000)
    # the float64 evaluation agrees wherever the float32 one neither saturates nor cancels: silence logits within +-6, where the naive
    # log(1 - sigmoid(x)) carries e^6 2^-24 = 2.4e-5 of rounding
    em64 = H.emissions(lg.double(), labels, n_labels, hi, var)
    calm = (lg[..., V - 1].abs() <= 6).unsqueeze(-1).expand_as(em) if var == H.CTC else torch.ones_like(em, dtype=torch.bool)
    assert int(calm.sum()) > em.numel() // 2 and H.rel_err(em[calm], em64[calm]) <= 1e-4


def test_logits_is_the_linear_layer():
    g = torch.Generator().manual_seed(1)
    act, w, b = (torch.randn(7, 32, generator=g, dtype=torch.float64), torch.randn(5, 32, generator=g, dtype=torch.float64),
                 torch.randn(5, generator=g, dtype=torch.float64))
    assert H.rel_err(H.logits(act, w, b), torch.nn.functional.linear(act, w, b)) <= TIGHT
    assert H.logits(act.float(), w.float(), b.float()).dtype == torch.float32


def test_silence_bracket_holds_two_float32_sigmoids():
    """torch's float32 sigmoid and the naive 1 / (1 + exp(-x)) in float32, then log(s) and log(1 - s) in float32: inside the bracket at
    every sweep value at or above -87 (log(1 - s) at every value); exactly -1000 for log(s) at x0 <= -89; -inf for log(1 - s) from 16.75
    on, which the bracket admits."""
    xs = H.sweep_values()
    assert not bool(((xs > -89) & (xs < -87)).any()) and float(xs.min()) == -104.0 and float(xs.max()) == 40.0
    for v in (-89.0, -87.0, 16.5, 16.75, 17.0, 17.5, -32.0, 32.0, 31.75, 0.25):
        assert v in xs.tolist()
    clamp = torch.tensor(-1000.0)
    forms = {"torch": torch.sigmoid(xs), "naive": 1.0 / (1.0 + torch.exp(-xs))}
    for name, s in forms.items():
        ls, lv = torch.maximum(torch.log(s), clamp), torch.maximum(torch.log(1.0 - s), clamp)
        for i, x0 in enumerate(xs.tolist()):
            (s_lo, s_hi), (v_lo, v_hi), saturated = H.silence_bracket(x0)
            assert s_lo <= s_hi and v_lo <= v_hi
            if x0 <= -89:
                assert float(ls[i]) == -1000.0, (name, x0)
            else:
                assert s_lo <= float(ls[i]) <= s_hi, (name, x0, float(ls[i]), s_lo, s_hi)
            assert v_lo <= float(lv[i]) <= v_hi, (name, x0, float(lv[i]), v_lo, v_hi)
            if x0 >= 16.75:
                assert float(lv[i]) == -1000.0 and v_lo == -1000.0, (name, x0)
            if saturated:
                assert float(lv[i]) == -1000.0
    # the bracket is tight where nothing cancels: a few ulps of the value
    (s_lo, s_hi), (v_lo, v_hi), _ = H.silence_bracket(0.0)
    assert s_hi - s_lo < 2e-6 and v_hi - v_lo < 2e-6 and s_lo < math.log(0.5) < s_hi
    (s_lo, s_hi), (v_lo, v_hi), _ = H.silence_bracket(-89.0)
    assert -1e-44 < v_lo <= 0.0 <= v_hi < 1e-44                      # log(1 - 0) = 0, widened by 4 ulps of zero


# ---- host-side argument checks ------------------------------------------------------------------------------------------------------

P = 4096                      # non-null, 256-byte aligned, never dereferenced
FC_ORDER = ("dtype", "act", "ld_act", "w_fc", "b_fc", "batch", "frames", "in_dim", "vocab", "variant", "labels", "labels_stride", "n_labels",
            "max_labels", "em", "em_batch_stride", "em_row_stride", "workspace", "workspace_bytes", "stream")
X2_ORDER = ("act", "ld_act", "w_fc", "b_fc", "w_x2", "w_x2s") + FC_ORDER[5:]
EL_ORDER = ("logits", "batch_stride", "row_stride", "batch", "frames", "vocab", "variant", "labels", "labels_stride", "n_labels", "max_labels",
            "em", "em_batch_stride", "em_row_stride", "stream")


def _lib():
    from lyricalignment_amd import _lib
    return _lib


def _fc_args(**kw):
    """A valid la_fc_emissions call on stand-in pointers (never launched: every test turns one argument into an invalid one)."""
    a = dict(dtype=0, act=P, ld_act=64, w_fc=P, b_fc=P, w_x2=P, w_x2s=P, batch=2, frames=10, in_dim=64, vocab=50, variant=1, labels=P,
             labels_stride=5, n_labels=P, max_labels=5, em=P, em_batch_stride=60, em_row_stride=6, workspace=P, workspace_bytes=None, stream=0)
    a.update(kw)
    return a


def _need(L, a, x2=False):
    need = ctypes.c_size_t(0)
    dims = [max(1, a[k]) for k in ("batch", "frames", "in_dim", "vocab", "max_labels")]
    rc = (L.la_fc_emissions_x2_workspace_bytes(*dims, ctypes.byref(need)) if x2 else
          L.la_fc_emissions_workspace_bytes(a["dtype"] if a["dtype"] in (0, 1, 2) else 0, *dims, ctypes.byref(need)))
    assert rc == 0
    return need.value


def _fc_call(L, a, x2=False):
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = _need(L, a, x2)
    if x2:
        return L.la_fc_emissions_x2(*[a[k] for k in X2_ORDER])
    return L.la_fc_emissions(*[a[k] for k in FC_ORDER])


FC_BAD = [
    (dict(act=0), "null pointer"), (dict(w_fc=0), "null pointer"), (dict(b_fc=0), "null pointer"), (dict(labels=0), "null pointer"),
    (dict(n_labels=0), "null pointer"), (dict(em=0), "null pointer"), (dict(workspace=0), "null pointer"),
    (dict(dtype=3), "bad dtype"), (dict(dtype=-1), "bad dtype"),
    (dict(batch=-1), "bad sizes"), (dict(frames=-3), "bad sizes"), (dict(max_labels=0, labels_stride=0), "bad sizes"),
    (dict(max_labels=-2), "bad sizes"), (dict(in_dim=0), "bad sizes"), (dict(in_dim=-64), "bad sizes"),
    (dict(vocab=2, variant=1), "vocab too small"), (dict(vocab=1, variant=0), "vocab too small"), (dict(vocab=0), "vocab too small"),
    (dict(em_row_stride=5), "strides smaller than max_labels"), (dict(labels_stride=4), "strides smaller than max_labels"),
    (dict(in_dim=48, ld_act=48), "must be a multiple of 32"), (dict(dtype=1, in_dim=96, ld_act=96), "must be a multiple of 64"),
    (dict(dtype=2, in_dim=32, ld_act=32), "must be a multiple of 64"),
    (dict(act=P + 4), "alignment"), (dict(w_fc=P + 8), "alignment"), (dict(workspace=P + 128), "alignment"),
    (dict(ld_act=66), "alignment"),                                   # float32: 264 bytes
    (dict(dtype=1, ld_act=68), "alignment"),                          # 16-bit: 136 bytes
    (dict(dtype=2, act=P + 2), "alignment"),
]


@pytest.mark.parametrize("x2", [False, True])
def test_fc_emissions_rejects_bad_arguments_on_the_host(x2):
    lib = _lib()
    L, E = lib.lib(), lib.LA_EINVAL
    for change, message in FC_BAD:
        if x2 and "dtype" in change:
            continue                                                  # the x2 entry is float32 by signature
        assert _fc_call(L, _fc_args(**change), x2) == E, change
        assert message in lib.last_error(), (change, lib.last_error())
    # one byte short, for every dtype, a shape of the 128-column kernels and one of the 256 x 256 kernels (the x2 entry: with the planes)
    for dtype in ((0,) if x2 else (0, 1, 2)):
        for shape in (dict(), dict(batch=3, frames=171, in_dim=256, vocab=16130, ld_act=256, em_batch_stride=171 * 6)):
            a = _fc_args(dtype=dtype, **shape)
            a["workspace_bytes"] = _need(L, a, x2) - 1
            assert _fc_call(L, a, x2) == E and "workspace too small" in lib.last_error(), (dtype, shape)
    if x2:
        # a workspace sized by the plain query is too small where the planes of act live in it
        a = _fc_args(batch=3, frames=171, in_dim=256, vocab=16130, ld_act=256, em_batch_stride=171 * 6)
        a["workspace_bytes"] = _need(L, a, False)
        assert _fc_call(L, a, True) == E and "workspace too small" in lib.last_error()
        for change in (dict(w_x2=0), dict(w_x2s=0), dict(w_x2=P + 8)):
            assert _fc_call(L, _fc_args(**change), True) == E, change
            assert "planes of W_fc" in lib.last_error()


def test_emissions_from_logits_rejects_bad_arguments_on_the_host():
    lib = _lib()
    L, E = lib.lib(), lib.LA_EINVAL
    base = dict(logits=P, batch_stride=500, row_stride=50, batch=2, frames=10, vocab=50, variant=1, labels=P, labels_stride=5, n_labels=P,
                max_labels=5, em=P, em_batch_stride=60, em_row_stride=6, stream=0)
    bad = [(dict(logits=0), "null pointer"), (dict(labels=0), "null pointer"), (dict(n_labels=0), "null pointer"), (dict(em=0), "null pointer"),
           (dict(batch=-1), "bad sizes"), (dict(frames=-1), "bad sizes"), (dict(max_labels=0), "bad sizes"), (dict(max_labels=-1), "bad sizes"),
           (dict(vocab=2, variant=1), "vocab too small"), (dict(vocab=1, variant=0), "vocab too small"), (dict(vocab=-5), "vocab too small"),
           (dict(em_row_stride=5), "em_row_stride < max_labels + 1")]
    for change, message in bad:
        a = dict(base, **change)
        assert L.la_emissions_from_logits(*[a[k] for k in EL_ORDER]) == E, change
        assert message in lib.last_error(), (change, lib.last_error())
    assert L.la_emissions_from_logits(*[dict(base, vocab=2, variant=1)[k] for k in EL_ORDER]) == E      # 2 columns are enough for plain only


def test_an_empty_batch_returns_before_any_pointer_is_looked_at():
    lib = _lib()
    L = lib.lib()
    nothing = dict(act=0, w_fc=0, b_fc=0, w_x2=P, w_x2s=P, labels=0, n_labels=0, em=0, workspace=0, workspace_bytes=0)
    for empty in (dict(batch=0), dict(frames=0)):
        for dtype in (0, 1, 2):
            assert _fc_call(L, _fc_args(dtype=dtype, **nothing, **empty)) == lib.LA_OK
        assert _fc_call(L, _fc_args(**nothing, **empty), True) == lib.LA_OK
        a = dict(logits=0, batch_stride=0, row_stride=0, batch=2, frames=10, vocab=50, variant=1, labels=0, labels_stride=0, n_labels=0,
                 max_labels=5, em=0, em_batch_stride=0, em_row_stride=0, stream=0)
        a.update(empty)
        assert L.la_emissions_from_logits(*[a[k] for k in EL_ORDER]) == lib.LA_OK


def test_workspace_queries():
    """Both queries reject non-positive sizes and a null result; they follow the stated layout (tests/head_reference.py workspace_layout),
    are monotone in each argument, and the x2 query adds exactly the planes of act and their scales inside the 256 x 256 kernel's domain
    and nothing outside it."""
    lib = _lib()
    L, E = lib.lib(), lib.LA_EINVAL
    need, need2 = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for bad in ((0, 10, 64, 50, 5), (2, 0, 64, 50, 5), (2, 10, 0, 50, 5), (2, 10, 64, 0, 5), (2, 10, 64, 50, 0), (-1, 10, 64, 50, 5)):
        assert L.la_fc_emissions_workspace_bytes(0, *bad, ctypes.byref(need)) == E and "fc_emissions_workspace_bytes" in lib.last_error()
        assert L.la_fc_emissions_x2_workspace_bytes(*bad, ctypes.byref(need)) == E and "fc_emissions_x2_workspace_bytes" in lib.last_error()
    assert L.la_fc_emissions_workspace_bytes(0, 2, 10, 64, 50, 5, None) == E and L.la_fc_emissions_x2_workspace_bytes(2, 10, 64, 50, 5, None) == E

    def q(dtype, *dims):
        assert L.la_fc_emissions_workspace_bytes(dtype, *dims, ctypes.byref(need)) == 0
        return need.value

    def q2(*dims):
        assert L.la_fc_emissions_x2_workspace_bytes(*dims, ctypes.byref(need2)) == 0
        return need2.value

    up = lambda n: (n + 255) // 256 * 256
    shapes = [(1, 1, 32, 2, 1), (5, 1, 32, 3, 7), (3, 43, 96, 300, 7), (3, 171, 128, 16130, 7), (3, 171, 256, 16130, 7), (2, 256, 256, 16130, 7),
              (3, 171, 256, 300, 7), (1, 4097, 64, 300, 7), (9, 1500, 256, 2000, 26), (3, 171, 384, 16129, 300)]
    for dims in shapes:
        B, T, K, V, Lm = dims
        for dtype, es in ((0, 4), (1, 2), (2, 2)):
            got = q(dtype, *dims)
            assert got == H.workspace_layout(B, T, K, V, Lm, es)["total"] and got % 256 == 0, (dtype, dims)
        inside = H.x2_domain(B * T, K, V)
        assert q2(*dims) == H.workspace_layout(B, T, K, V, Lm, 4, inside)["total"]
        extra = q2(*dims) - q(0, *dims)
        assert extra == (up(B * T * 2 * K * 2) + up(B * T * 4) if inside else 0), dims
        for i in range(5):                               # monotone in each argument
            more = list(dims)
            more[i] += 1 if i != 2 else 128
            assert q(0, *more) >= q(0, *dims) and q(1, *more) >= q(1, *dims)
            if H.x2_domain(more[0] * more[1], more[2], more[3]) >= inside:
                assert q2(*more) >= q2(*dims)
            assert q2(*more) >= q(0, *more)
    assert [H.x2_domain(d[0] * d[1], d[2], d[3]) for d in shapes] == [False, False, False, False, True, False, False, False, True, True]
