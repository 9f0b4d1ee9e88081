"""The restatement of the GRU recurrence (tests/gru_reference.py) pinned to torch.nn.GRU and to torch autograd in float64, the
properties the GPU tests rely on checked on the CPU (every generated case has a non-zero float32 yardstick unless declared degenerate;
the float32 restatement passes the 16-bit assertion against the float64 one), and every host-side rejection of la_gru_layer,
la_gru_layer_ragged, la_gru_layer_train_fwd, la_gru_layer_bwd and la_gru_workspace_bytes through the C ABI.  Runs without a GPU: the
rejected calls carry stand-in pointers and must come back before any launch."""
import ctypes

import pytest
import torch

import gru_reference as G

TIGHT = 1e-12        # two float64 evaluations of the same formulas
P = 4096             # non-null, 256-byte aligned, never dereferenced
FACTOR = 8.0


@pytest.mark.parametrize("T", [1, 2, 37])
@pytest.mark.parametrize("kind", ["gauss", "trained", "sat"])
def test_driven_restatement_reproduces_nn_gru_in_float64(T, kind):
    """Free-running, and driven by its own unrounded output, the restatement is torch.nn.GRU to float64 accuracy in both directions;
    driven by its own ROUNDED output it reproduces the free run that rounds its exchanged copy (the 16-bit kernels' arithmetic)."""
    B, H = 3, 64
    gi, w, b = G.forward_case(kind, B, T, H)
    with torch.no_grad():
        # (the module multiplies gi with its identity input weights: inf x 0 is NaN there, so it is fed +-1e5, which has the same limits)
        ref = G.torch_gru(gi.clamp(-1e5, 1e5), w, b)[0].reshape(B, T, 2, H)
    for forced in (False, True):                      # driven by the module's output: the module, step by step
        by_ref = G.driven_forward(gi, w, b, exch=ref.reshape(B, T, 2 * H), carry_from_exch=forced)
        assert float((by_ref["h"] - ref).abs().max()) <= TIGHT
        assert float((by_ref["mish"] - torch.nn.functional.mish(ref)).abs().max()) <= TIGHT
    free = G.driven_forward(gi, w, b)
    if kind != "trained":                             # (W_hh ~ N(0, 1) is a chaotic map: a free run 37 steps long multiplies 1e-16 to 1e-7)
        assert float((free["h"] - ref).abs().max()) <= TIGHT
        assert float((free["mish"] - torch.nn.functional.mish(ref)).abs().max()) <= TIGHT
    assert not any(bool(torch.isnan(v).any()) for v in free.values())
    for forced in (False, True):
        driven = G.driven_forward(gi, w, b, exch=free["h"].reshape(B, T, 2 * H), carry_from_exch=forced)
        for k in G.OUTPUTS:
            assert float((driven[k] - free[k]).abs().max()) <= TIGHT, k
    for dt in ("bf16", "f16"):
        rounded = G.driven_forward(gi, w, b, round_to=G.TYPES[dt])
        exch = rounded["h"].to(G.TYPES[dt]).reshape(B, T, 2 * H)
        driven = G.driven_forward(gi, w, b, exch=exch)
        for k in G.OUTPUTS:
            assert float((driven[k] - rounded[k]).abs().max()) <= TIGHT, (dt, k)
    if kind == "sat":
        # the limits are exact: 0, 1, +-1
        r, z, n = free["r"], free["z"], free["n"]
        assert bool((r[..., 24:28] == 1).all()) and bool((r[..., 28:32] == 0).all()) and bool((r[..., 44:48] == 1).all()) and bool((r[..., 48:52] == 0).all())
        assert bool((z[..., 52:56] == 0).all()) and bool((n[..., 56:60] == 1).all()) and bool((n[..., 60:64] == -1).all())
        if T > 4:
            assert bool((z[:, 2:T - 2, :, 32:36] == 1).all())
            assert torch.equal(free["h"][:, 2, 0, 32:36], free["h"][:, 1, 0, 32:36]) and bool((free["h"][:, 1, 0, 32:36] != 0).all())


def test_ragged_restatement_is_each_clip_alone():
    B, T, H = 6, 9, 64
    gi, w, b = G.forward_case("gauss", B, T, H)
    nf = G.ragged_lengths(B, T)
    assert nf.tolist()[:4] == [T, 1, 2, T - 1]
    got = G.driven_forward(G.with_nan_past_the_end(gi, nf), w, b, n_frames=nf)
    for bb, n in enumerate(nf.tolist()):
        alone = G.driven_forward(gi[bb:bb + 1, :n], w, b)
        for k in ("h", "mish"):
            assert float((got[k][bb, :n] - alone[k][0]).abs().max()) <= TIGHT
        assert bool((got["h"][bb, n:] == 0).all())


@pytest.mark.parametrize("T", [1, 2, 37])
def test_backward_restatement_matches_autograd_through_nn_gru(T):
    """gi is the leaf nn.GRU reads (identity input weights): its gradient is dgi; the bias and weight gradients of the recurrent side are
    the sums of dgh and of dgh^T h_prev."""
    B, H = 3, 64
    gi, w, b = G.forward_case("gauss", B, T, H)
    out, x, gru = G.torch_gru(gi, w, b)
    dout = torch.randn(B, T, 2 * H, generator=torch.Generator().manual_seed(T), dtype=torch.float64)
    out.backward(dout)
    f = G.driven_forward(gi, w, b)
    gates = torch.cat([f["r"], f["z"], f["n"], f["hn"]], -1)
    dgi, dgh = G.backward(gates, f["h"].reshape(B, T, 2 * H), dout, w)
    assert float((dgi.reshape(B, T, 6 * H) - x.grad).abs().max()) <= TIGHT * max(1.0, float(x.grad.abs().max()))
    for d, (bias, wt) in enumerate(((gru.bias_hh_l0, gru.weight_hh_l0), (gru.bias_hh_l0_reverse, gru.weight_hh_l0_reverse))):
        assert float((dgh[:, :, d].sum((0, 1)) - bias.grad).abs().max()) <= 1e-10
        hp = torch.zeros(B, T, H, dtype=torch.float64)
        if d == 0:
            hp[:, 1:] = f["h"][:, :-1, 0]
        else:
            hp[:, :-1] = f["h"][:, 1:, 1]
        assert float((torch.einsum("btj,btk->jk", dgh[:, :, d], hp) - wt.grad).abs().max()) <= 1e-10


def _yardsticks(kind, B, T, H, wdt):
    gi, w, b = G.forward_case(kind, B, T, H, wdt)
    rt = None if wdt == "f32" else G.TYPES[wdt]
    exch = G.driven_forward(gi, w, b, round_to=rt)["h"].reshape(B, T, 2 * H)
    if rt is not None:
        exch = exch.to(rt)
    r64 = G.driven_forward(gi, w, b, exch=exch, carry_from_exch=rt is None)
    r32 = G.driven_forward(gi, w, b, exch=exch, carry_from_exch=rt is None, dtype=torch.float32)
    return r64, r32, G.e32_step(r64, r32)


@pytest.mark.parametrize("wdt", ["f32", "bf16", "f16"])
def test_every_generated_case_has_a_yardstick(wdt):
    """E32_step > 0 for every output of every case but the declared degenerate ones, which are exactly zero and fall back to the
    Gaussian base case of the same shape; the backward cases likewise."""
    B, T, H = 5, 37, 64
    for kind in G.FWD_CASES:
        _, r32, e = _yardsticks(kind, B, T, H, wdt)
        assert r32["h"].dtype == torch.float32
        for k in G.OUTPUTS:
            if k in G.FWD_DEGENERATE.get(kind, ()):
                assert e[k] == 0.0, (kind, k)
            else:
                assert e[k] > 0.0, (kind, k)
    if wdt == "f32":
        for kind in G.BWD_CASES:
            gates, out, dout, w = G.backward_case(kind, B, T, H)
            r64, r32 = G.backward(gates, out, dout, w), G.backward(gates, out, dout, w, torch.float32)
            for a, c in zip(r64, r32):
                assert (G.rel_max(c, a) == 0.0) == (kind in G.BWD_DEGENERATE), kind
                assert G.rel_max(c, a) < 1e-5


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_the_float32_restatement_passes_the_16_bit_assertion(dt):
    """The reference alone passes its own test: the float32 restatement rounded to the type lies within ulp_T(ref) / 2 + 8 E32_step of
    the float64 one in every element of every case."""
    B, T, H = 5, 37, 64
    base = _yardsticks("gauss", B, T, H, dt)[2]
    for kind in G.FWD_CASES:
        r64, r32, e = _yardsticks(kind, B, T, H, dt)
        for k in ("h", "mish"):
            got = r32[k].to(G.TYPES[dt]).double()
            bound = 0.5 * G.ulp_T(r64[k], dt) + FACTOR * (e[k] if e[k] > 0 else base[k])
            assert bool(((got - r64[k]).abs() <= bound).all()), (kind, k)


def test_ulp_of_the_16_bit_types():
    x = torch.tensor([1.0, 0.75, 0.5, 0.49, 3e-5, 0.0, -1.0, 1e-40], dtype=torch.float64)
    assert G.ulp_T(x, "f16").tolist() == [2.0 ** -10, 2.0 ** -11, 2.0 ** -11, 2.0 ** -12, 2.0 ** -26 * 4, 2.0 ** -24, 2.0 ** -10, 2.0 ** -24]
    assert G.ulp_T(x, "bf16").tolist()[:4] == [2.0 ** -7, 2.0 ** -8, 2.0 ** -8, 2.0 ** -9] and float(G.ulp_T(x, "bf16")[5]) == 2.0 ** -133
    for dt in ("bf16", "f16"):                                  # against the type itself: the next value up
        v = torch.tensor([1.0, 0.3, 0.007], dtype=G.TYPES[dt])
        nxt = (v.view(torch.int16) + 1).view(G.TYPES[dt])
        assert torch.equal((nxt.double() - v.double()), G.ulp_T(v.double(), dt))


# ---- host-side argument checks ------------------------------------------------------------------------------------------------------

FWD_ORDER = ("dtype", "gi", "w_hh", "b_hh", "out", "out_mish", "batch", "frames", "hidden", "workspace", "workspace_bytes", "timeout_flag", "stream")
RAG_ORDER = FWD_ORDER[:8] + ("n_frames",) + FWD_ORDER[8:]
TRAIN_ORDER = ("gi", "w_hh", "b_hh", "out", "gates", "batch", "frames", "hidden", "workspace", "workspace_bytes", "timeout_flag", "stream")
BWD_ORDER = ("gates", "out", "dout", "w_hh", "dgi", "dgh", "batch", "frames", "hidden", "workspace", "workspace_bytes", "timeout_flag", "stream")


def _lib():
    from lyricalignment_amd import _lib
    return _lib


def _args(**kw):
    a = dict(dtype=0, gi=P, w_hh=P, b_hh=P, out=P, out_mish=0, gates=P, dout=P, dgi=P, dgh=P, n_frames=P, batch=3, frames=5, hidden=64,
             workspace=P, workspace_bytes=None, timeout_flag=0, stream=0)
    a.update(kw)
    return a


def _call(entry, a):
    lib = _lib()
    L = lib.lib()
    if a["workspace_bytes"] is None:
        need = ctypes.c_size_t(0)
        assert L.la_gru_workspace_bytes(max(1, a["batch"]), max(1, a["frames"]), max(1, a["hidden"]), ctypes.byref(need)) == 0
        a["workspace_bytes"] = need.value + a.pop("short", 0)
    fn, order = {"fwd": (L.la_gru_layer, FWD_ORDER), "ragged": (L.la_gru_layer_ragged, RAG_ORDER),
                 "train": (L.la_gru_layer_train_fwd, TRAIN_ORDER), "bwd": (L.la_gru_layer_bwd, BWD_ORDER)}[entry]
    return fn(*[a[k] for k in order]), lib.last_error()


FORWARD_BAD = [
    (dict(gi=0), "null pointer"), (dict(w_hh=0), "null pointer"), (dict(b_hh=0), "null pointer"), (dict(out=0), "null pointer"),
    (dict(workspace=0), "null pointer"),
    (dict(batch=-1), "bad sizes"), (dict(frames=-2), "bad sizes"), (dict(hidden=0), "bad sizes"), (dict(hidden=-64), "bad sizes"),
    (dict(w_hh=P + 8), "alignment"), (dict(out=P + 4), "alignment"), (dict(workspace=P + 8), "alignment"),
    (dict(short=-1), "workspace too small"), (dict(short=-1, batch=17, frames=37, hidden=384), "workspace too small"),
]


@pytest.mark.parametrize("entry", ["fwd", "ragged", "train"])
def test_forward_entries_reject_bad_arguments_on_the_host(entry):
    lib = _lib()
    for change, message in FORWARD_BAD:
        rc, err = _call(entry, _args(**change))
        assert rc == lib.LA_EINVAL and message in err, (change, rc, err)
    if entry != "train":
        for d in (3, -1):
            rc, err = _call(entry, _args(dtype=d))
            assert rc == lib.LA_EINVAL and "bad dtype" in err
    if entry == "ragged":
        rc, err = _call(entry, _args(n_frames=0))
        assert rc == lib.LA_EINVAL and "n_frames missing" in err
    if entry == "train":
        rc, err = _call(entry, _args(gates=0))
        assert rc == lib.LA_EINVAL and "gates buffer missing" in err


def test_backward_rejects_bad_arguments_on_the_host():
    lib = _lib()
    bad = [(dict(gates=0), "null pointer"), (dict(out=0), "null pointer"), (dict(dout=0), "null pointer"), (dict(w_hh=0), "null pointer"),
           (dict(dgi=0), "null pointer"), (dict(dgh=0), "null pointer"), (dict(workspace=0), "null pointer"),
           (dict(batch=-1), "bad sizes"), (dict(frames=-2), "bad sizes"), (dict(hidden=0), "bad sizes"),
           (dict(dgh=P + 8), "alignment"), (dict(workspace=P + 8), "alignment"),
           (dict(short=-1), "workspace too small"), (dict(short=-1, batch=17, frames=37, hidden=384), "workspace too small")]
    for change, message in bad:
        rc, err = _call("bwd", _args(**change))
        assert rc == lib.LA_EINVAL and message in err, (change, rc, err)


def test_an_unsupported_hidden_size_is_the_same_status_forward_and_backward():
    """A well-formed hidden size the kernels are not built for is LA_EUNSUPPORTED in every entry (include/lyricalign.h): not a multiple
    of 64; float32 above 384, 16-bit above 512, backward above 384.  The limits themselves are not rejected for their size: with a
    workspace one byte short they get as far as that check."""
    lib = _lib()
    U = lib.LA_EUNSUPPORTED
    for entry, dtype, hs in (("fwd", 0, (96, 32, 448, 512)), ("fwd", 1, (96, 576, 1024)), ("fwd", 2, (32, 576)), ("ragged", 0, (448,)),
                             ("ragged", 1, (576,)), ("train", 0, (96, 448)), ("bwd", 0, (96, 32, 448, 512))):
        for h in hs:
            rc, err = _call(entry, _args(dtype=dtype, hidden=h))
            assert rc == U and f"hidden={h} unsupported" in err, (entry, dtype, h, rc, err)
    for entry, dtype, h in (("fwd", 0, 384), ("fwd", 1, 512), ("fwd", 2, 512), ("train", 0, 384), ("bwd", 0, 384)):
        rc, err = _call(entry, _args(dtype=dtype, hidden=h, short=-1))
        assert rc == lib.LA_EINVAL and "workspace too small" in err


def test_the_co_residency_cap_at_the_smallest_batch_that_crosses_it():
    """nsplit 2 groups > 224 workgroups: float32 (2-wave workgroups, nsplit = H / 32) at H = 384 from 145 clips; 16-bit 4-wave
    (nsplit = H / 64) at H = 512 from 225; 16-bit 8-wave (nsplit = H / 128) at H = 384 from 593; the backward's f16x2 form
    (H / 64 workgroups) at H = 384 takes 288 clips, its float32 form (option gru_handoff = 1, H / 32) 144."""
    lib = _lib()
    U = lib.LA_EUNSUPPORTED

    def crossing(nsplit):
        return 16 * (224 // (2 * nsplit)) + 1

    assert [crossing(12), crossing(8), crossing(3), crossing(6)] == [145, 225, 593, 289]
    for entry, dtype, h, b in (("fwd", 0, 384, 145), ("train", 0, 384, 145), ("ragged", 0, 384, 145), ("fwd", 1, 512, 225), ("fwd", 2, 512, 225),
                               ("fwd", 1, 384, 593), ("ragged", 2, 384, 593), ("bwd", 0, 384, 289)):
        rc, err = _call(entry, _args(dtype=dtype, hidden=h, batch=b))
        assert rc == U and "co-resident workgroups needed" in err, (entry, dtype, h, b, rc, err)
        rc, err = _call(entry, _args(dtype=dtype, hidden=h, batch=b - 1, short=-1))         # one clip fewer: as far as the workspace check
        assert rc == lib.LA_EINVAL and "workspace too small" in err
    with lib.option("gru_handoff", 1):
        rc, err = _call("bwd", _args(hidden=384, batch=145))
        assert rc == U and "co-resident workgroups needed" in err
    with lib.option("gru_nw", 4):
        rc, err = _call("fwd", _args(dtype=1, hidden=384, batch=16 * (224 // 12) + 1))
        assert rc == U and "co-resident workgroups needed" in err


def test_an_empty_batch_returns_before_any_pointer_is_looked_at():
    lib = _lib()
    nothing = dict(gi=0, w_hh=0, b_hh=0, out=0, gates=0, dout=0, dgi=0, dgh=0, n_frames=0, workspace=0, workspace_bytes=0, hidden=7, dtype=9)
    for empty in (dict(batch=0), dict(frames=0)):
        for entry in ("fwd", "ragged", "train", "bwd"):
            rc, _ = _call(entry, _args(**nothing, **empty))
            assert rc == lib.LA_OK, (entry, empty)


def test_workspace_query_follows_its_documented_layout():
    lib = _lib()
    L = lib.lib()
    need = ctypes.c_size_t(0)
    for bad in ((0, 5, 64), (3, 0, 64), (3, 5, 0), (-1, 5, 64), (3, -5, 64), (3, 5, -64)):
        assert L.la_gru_workspace_bytes(*bad, ctypes.byref(need)) == lib.LA_EINVAL and "gru_workspace_bytes" in lib.last_error()
    assert L.la_gru_workspace_bytes(3, 5, 64, None) == lib.LA_EINVAL
    for B in (1, 4, 5, 15, 16, 17, 33, 144, 593):
        for T in (1, 2, 37, 59, 60, 1500):
            for H in (64, 96, 100, 128, 192, 256, 320, 384, 448, 512, 1):
                assert L.la_gru_workspace_bytes(B, T, H, ctypes.byref(need)) == 0
                lay = G.workspace_layout(B, T, H)
                assert need.value == lay["total"] and lay["ring"] % 256 == 0, (B, T, H, need.value, lay)
    # the backward ring is the larger one from H = 128 on, the forward ring at H = 64 and where H is no multiple of 64
    assert [G.workspace_layout(5, 37, h)["bwd_ring"] > G.workspace_layout(5, 37, h)["fwd_ring"] for h in (64, 96, 128, 384)] == [False, False, True, True]
