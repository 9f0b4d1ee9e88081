"""The GRU recurrence kernels (csrc/la_gru.hip) against the driven float64 restatement of tests/gru_reference.py, through the C ABI, one
step at a time: the recurrent product of every step is formed from the kernel's own `out` row of the step before, so a rounding flip of
an exchanged h is an input of the next step and not an error of it, and each step is held to the accuracy of its own arithmetic.

    form  kernel                                   selected when
    F1    gru_kernel<float>                        f32 la_gru_layer, B <= 4, or option gru_handoff = 1
    F2    gru_train_x2_kernel, no gates            f32 la_gru_layer, B > 4
    F3    gru_train_x2_kernel, gates               la_gru_layer_train_fwd
    F4    gru_kernel<float>, gates                 la_gru_layer_train_fwd, gru_handoff = 1
    F5    gru_kernel<16-bit>, 4 waves              H in {64, 192, 320, 448, 512}, or gru_nw = 4
    F6    gru_kernel<16-bit>, 8 waves, counters    H in {128, 256, 384}, B <= 16 or gru_handoff = 1
    F7    gru_granule_kernel                       H in {128, 256, 384}, B > 16 or gru_handoff = 2
    B1    gru_bwd_x2_kernel<H / 64>                la_gru_layer_bwd, B > 4
    B2    gru_bwd_kernel                           la_gru_layer_bwd, B <= 4 or gru_handoff = 1
An option is set only where the documented dispatch would pick another form, so the boundaries B = 4 / 5 and 16 / 17 are observed.

Set-up of every call: out, out_mish, gates, dgi and dgh each sit inside a sentinel-filled Guard; the workspace is exactly the queried size
between sentinel bytes; timeout_flag must stay 0.  Which form ran is observed: one launch of the timer family (gru_f32, gru_bf16,
gru_bwd_f32) and what the call left in the workspace -- the counter forms zero the counter region and leave `nsplit` arrivals in every
counter (H / 32 float32, H / 64 four-wave, H / 128 eight-wave: this tells F5 from F6) and never touch the ring; the granule forms zero only
the 16-byte header and the ring and leave step tags there (16 x H / 2 granules per slot for F7, 16 x H for F2 / F3, (H / 64)^2 blocks with
an empty diagonal for B1); gru_bwd_kernel zeroes the whole workspace.  F2 and F3 differ in the gates they were asked for.  The fence
variants (gru_fence = 1) leave the same traces as the write-through ones: they are pinned by the option alone and must give the same bits.

Assertions (FACTOR = 8 of tests/test_gpu_row_kernels.py; E32_step = |float32 restatement - float64 restatement|, largest over the case,
per output; where it is 0 the Gaussian case of the same shape lends its value):
    float32 outputs:  |got - ref| <= 8 E32_step
    16-bit outputs:   |got - ref| <= ulp_T(ref) / 2 + 8 E32_step        (every element)
    backward:         max |got - ref| / max |ref| <= 8 E32, for dgi and dgh separately
Every comparison prints `form/type case:output err E32 ratio` (16-bit: err is the excess over ulp / 2); the lines of one MI355X run are
kept in profiles/gru_kernel_errors.txt.  No form needed a term beyond 8 x E32_step: worst ratios F1 2.2, F2 1.4, F3 3.8, F4 3.7, 16-bit
forms 0.7, B1 1.8, B2 2.3.  Every kernel prefetches gi one step ahead, so T = 2 and 3 already cross that distance; T = 3
reuses a ring slot; T = 1 runs no hand-off.
"""
import contextlib
import ctypes
import functools
import math

import pytest
import torch

import gru_reference as G
from test_gpu_head_kernels import _count_launches, _Workspace
from test_gpu_row_kernels import FACTOR, Guard, _bits, _dev, _L, _ok, _st

pytestmark = pytest.mark.gpu

DT = {"f32": (torch.float32, 0), "bf16": (torch.bfloat16, 1), "f16": (torch.float16, 2)}
SENT32 = 0x5A5A5A5A
ALL_B = (1, 4, 5, 15, 16, 17, 33)
H64 = (64, 128, 192, 256, 320, 384)
T0 = 37


def _opts_f1(B, H): return {"gru_handoff": 1} if B > 4 else {}
def _opts_none(B, H): return {}
def _opts_f4(B, H): return {"gru_handoff": 1}
def _opts_f5(B, H): return {"gru_nw": 4} if H % 128 == 0 and H <= 384 else {}
def _opts_f6(B, H): return {"gru_handoff": 1} if B > 16 else {}
def _opts_f7(B, H): return {"gru_handoff": 2} if B <= 16 else {}
def _opts_b2(B, H): return {"gru_handoff": 1} if B > 4 else {}


# entry, types, options, hidden sizes, batch of the H sweep, batches of the B sweep, (trace kind, hidden units per workgroup)
FORMS = {
    "F1": ("layer", ("f32",), _opts_f1, H64, 3, ALL_B, ("counter", 32)),
    "F2": ("layer", ("f32",), _opts_none, H64, 5, ALL_B[2:], ("x2", 64)),
    "F3": ("train", ("f32",), _opts_none, H64, 5, ALL_B, ("x2", 64)),
    "F4": ("train", ("f32",), _opts_f4, H64, 3, ALL_B, ("counter", 32)),
    "F5": ("layer", ("bf16", "f16"), _opts_f5, H64 + (448, 512), 5, ALL_B, ("counter", 64)),
    "F6": ("layer", ("bf16", "f16"), _opts_f6, (128, 256, 384), 5, ALL_B, ("counter", 128)),
    "F7": ("layer", ("bf16", "f16"), _opts_f7, (128, 256, 384), 17, ALL_B, ("granule", 128)),
}
FORM_DT = [(f, dt) for f, spec in FORMS.items() for dt in spec[1]]
BWD = {"B1": (_opts_none, 5, ALL_B[2:]), "B2": (_opts_b2, 3, ALL_B)}


@contextlib.contextmanager
def _options(opts):
    from lyricalignment_amd import _lib
    with contextlib.ExitStack() as st:
        for k, v in opts.items():
            st.enter_context(_lib.option(k, v))
        yield


# ---- what a call leaves in the workspace --------------------------------------------------------------------------------------------

def _words(b):
    return b.contiguous().view(torch.int32)


def _tags_ok(tags, per_slot, last_step):
    """tags [pairs of (group, direction)][2 slots][per_slot]: the slot of the last published step carries last_step + 1, the other one
    last_step (0: never written)."""
    t = tags.reshape(-1, 2, per_slot)
    want = [0, 0]
    if last_step >= 0:
        want[last_step & 1] = last_step + 1
        want[(last_step & 1) ^ 1] = last_step
    return bool((t[:, 0] == want[0]).all()) and bool((t[:, 1] == want[1]).all())


def _observe(wsb, B, T, H):
    """-> ('counter', arrivals, ring state) or ('granule', ring words) from the bytes of the workspace after the call."""
    lay = G.workspace_layout(B, T, H)
    assert lay["total"] == wsb.numel()
    off, n = lay["counters"]
    assert bool((_words(wsb[:16]) == 0).all()), "the header was not zeroed"
    ctr, pad, ring = _words(wsb[off: off + 4 * n]), wsb[off + 4 * n: lay["ring"]], _words(wsb[lay["ring"]:])
    if bool((ctr == SENT32).all()):
        assert bool((pad == 0x5A).all())
        return ("granule", ring)
    assert bool((pad == 0).all()) and len(set(ctr.tolist())) == 1, "arrival counters differ"
    state = "zero" if bool((ring == 0).all()) else ("untouched" if bool((ring == SENT32).all()) else "mixed")
    return ("counter", int(ctr[0]), state)


def _expect_trace(name, wsb, B, T, H, trace):
    kind, per_wg = trace
    lay = G.workspace_layout(B, T, H)
    obs = _observe(wsb, B, T, H)
    groups = lay["groups"]
    if kind == "counter":
        assert obs == ("counter", H // per_wg, "untouched"), (name, obs[:3])
    elif kind == "bwd_counter":
        assert obs == ("counter", H // 32, "zero"), (name, obs[:3])
    else:
        assert obs[0] == "granule", (name, obs[:3])
        ring = obs[1]
        if kind == "bwd_x2":
            ns = H // 64
            used = lay["bwd_ring"] // 4
            tags = ring[:used][1::2].reshape(groups * 2, 2, ns, ns, 1024)
            diag = torch.eye(ns, dtype=torch.bool)
            assert bool((tags[:, :, diag] == 0).all()) and bool((ring[:used][0::2].reshape(groups * 2, 2, ns, ns, 1024)[:, :, diag] == 0).all())
            if ns > 1:
                assert _tags_ok(tags[:, :, ~diag].reshape(groups * 2, 2, -1), (ns * ns - ns) * 1024, T - 2), name
        else:
            per_slot = 16 * (H // 2 if kind == "granule" else H)
            used = groups * 2 * 2 * per_slot * 2
            assert _tags_ok(ring[:used][1::2], per_slot, T - 1), (name, "step tags")
            zeroed = lay["fwd_ring"] // 4
            assert bool((ring[used:zeroed] == 0).all())
        assert bool((ring[zeroed if kind != "bwd_x2" else used:] == SENT32).all()), (name, "written past its ring")


# ---- one call -----------------------------------------------------------------------------------------------------------------------

class _Run:
    pass


def _forward(name, entry, dt, gi, w, b, opts, trace, n_frames=None):
    L = _L()
    dtype, code = DT[dt]
    B, T, _, H3 = gi.shape
    H = H3 // 3
    gid, wd, bd = _dev(gi), _dev(w.to(dtype)), _dev(b)
    out = Guard((B, T, 2 * H), dtype=dtype)
    outm = Guard((B, T, 2 * H), dtype=dtype) if entry != "train" else None
    gates = Guard((B, T, 2, 4 * H)) if entry == "train" else None
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    need = ctypes.c_size_t(0)
    _ok(L.la_gru_workspace_bytes(B, T, H, ctypes.byref(need)), "workspace query")
    ws = _Workspace(need.value)
    nfd = _dev(n_frames) if n_frames is not None else None
    with _options(opts), _count_launches("gru_f32" if dt == "f32" else "gru_bf16") as c:
        if entry == "train":
            rc = L.la_gru_layer_train_fwd(gid.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.ptr, gates.ptr, B, T, H, ws.ptr, need.value,
                                          flag.data_ptr(), _st())
        elif n_frames is not None:
            rc = L.la_gru_layer_ragged(code, gid.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.ptr, outm.ptr, B, T, nfd.data_ptr(), H, ws.ptr,
                                       need.value, flag.data_ptr(), _st())
        else:
            rc = L.la_gru_layer(code, gid.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.ptr, outm.ptr, B, T, H, ws.ptr, need.value,
                                flag.data_ptr(), _st())
        _ok(rc, name)
    assert c.n == 1, (name, c.n)
    assert int(flag.item()) == 0, f"{name}: a bounded wait timed out"
    r = _Run()
    out.check()
    r.out = out.get()
    r.mish = r.gates = None
    if outm is not None:
        outm.check()
        r.mish = outm.get()
    if gates is not None:
        gates.check()
        r.gates = gates.get()
    _expect_trace(name, ws.check(), B, T, H, trace)
    return r


def _backward(name, gates, out, dout, w, opts, trace):
    L = _L()
    B, T, _, H4 = gates.shape
    H = H4 // 4
    gd, od, dd, wd = _dev(gates), _dev(out), _dev(dout), _dev(w)
    dgi, dgh = Guard((B, T, 2, 3 * H)), Guard((B, T, 2, 3 * H))
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    need = ctypes.c_size_t(0)
    _ok(L.la_gru_workspace_bytes(B, T, H, ctypes.byref(need)), "workspace query")
    ws = _Workspace(need.value)
    with _options(opts), _count_launches("gru_bwd_f32") as c:
        _ok(L.la_gru_layer_bwd(gd.data_ptr(), od.data_ptr(), dd.data_ptr(), wd.data_ptr(), dgi.ptr, dgh.ptr, B, T, H, ws.ptr, need.value,
                               flag.data_ptr(), _st()), name)
    assert c.n == 1, (name, c.n)
    assert int(flag.item()) == 0, f"{name}: a bounded wait timed out"
    dgi.check(); dgh.check()
    _expect_trace(name, ws.check(), B, T, H, trace)
    return dgi.get(), dgh.get()


# ---- comparisons --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _base_e32(dt, B, T, H):
    """E32_step of the Gaussian case of the shape, driven by the free-running restatement's own (rounded) output: lent to the outputs of
    a case whose own yardstick is exactly zero."""
    gi, w, b = G.forward_case("gauss", B, T, H, dt)
    rt = None if dt == "f32" else G.TYPES[dt]
    exch = G.driven_forward(gi, w, b, round_to=rt)["h"].reshape(B, T, 2 * H)
    exch = exch if rt is None else exch.to(rt)
    kw = dict(exch=exch, carry_from_exch=rt is None)
    return G.e32_step(G.driven_forward(gi, w, b, **kw), G.driven_forward(gi, w, b, dtype=torch.float32, **kw))


def _compare_forward(name, dt, case, run, gi, w, b, n_frames=None, clips=None):
    """Every written element of the checked rows (ragged: t < n_frames[b]; clips: those clips only) against the driven restatement.
    -> the list of failures (all lines are printed first)."""
    B, T, _, H3 = gi.shape
    H = H3 // 3
    kw = dict(exch=run.out, n_frames=n_frames, carry_from_exch=dt == "f32")
    r64 = G.driven_forward(gi, w, b, **kw)
    r32 = G.driven_forward(gi, w, b, dtype=torch.float32, **kw)
    mask = torch.ones(B, T, dtype=torch.bool)
    if n_frames is not None:
        mask &= torch.arange(T).reshape(1, T) < n_frames.reshape(B, 1)
    if clips is not None:
        keep = torch.zeros(B, dtype=torch.bool)
        keep[list(clips)] = True
        mask &= keep.reshape(B, 1)
    e32, base = G.e32_step(r64, r32, mask), _base_e32(dt, B, T, H)
    got = {"h": run.out.reshape(B, T, 2, H)}
    if run.mish is not None:
        got["mish"] = run.mish.reshape(B, T, 2, H)
    if run.gates is not None:
        for i, k in enumerate(("r", "z", "n", "hn")):
            got[k] = run.gates[..., i * H:(i + 1) * H]
    bad = []
    for k, gv in got.items():
        g, ref = gv.double()[mask], r64[k][mask]
        assert not bool(torch.isnan(ref).any())
        if not bool(torch.isfinite(g).all()):
            bad.append((name, case, k, "non-finite output"))
            continue
        e = e32[k] if e32[k] > 0 else base[k]
        slack = 0.5 * G.ulp_T(ref, dt) if dt != "f32" else torch.zeros_like(ref)
        err = float(((g - ref).abs() - slack).clamp(min=0).max())
        # (e == 0 even in the Gaussian case: hn = b_hn at T = 1, exact in every arithmetic -- then the kernel's must be exact too)
        print(f"{name}/{dt} {case}:{k} {err:.3e} {e:.3e} {_ratio(err, e):.2f}")
        if not err <= FACTOR * e:
            bad.append((name, case, k, err, e))
    return bad


def _ratio(err, e):
    return err / e if e > 0 else (0.0 if err == 0 else math.inf)


def _compare_backward(name, case, got, gates, out, dout, w, clips=None):
    B, T, _, H4 = gates.shape
    r64, r32 = G.backward(gates, out, dout, w), G.backward(gates, out, dout, w, torch.float32)
    bg = G.backward_case("gauss", B, T, H4 // 4)
    base = [G.rel_max(a, c) for a, c in zip(G.backward(*bg, torch.float32), G.backward(*bg))]
    bad = []
    for k, g, a, c, be in zip(("dgi", "dgh"), got, r64, r32, base):
        if clips is not None:
            g, a, c = g[list(clips)], a[list(clips)], c[list(clips)]
        if not bool(torch.isfinite(g).all()):
            bad.append((name, case, k, "non-finite output"))
            continue
        err, e = G.rel_max(g, a), G.rel_max(c, a)
        e = e if e > 0 else be
        print(f"{name}/f32 {case}:{k} {err:.3e} {e:.3e} {_ratio(err, e):.2f}")
        if not err <= FACTOR * e:
            bad.append((name, case, k, err, e))
    return bad


def _one(form, dt, case, B, T, H, *, ragged=False, fence=False):
    entry, _, optf, _, _, _, trace = FORMS[form]
    gi, w, b = G.forward_case(case, B, T, H, dt)
    nf = G.ragged_lengths(B, T) if ragged else None
    if ragged:
        gi = G.with_nan_past_the_end(gi, nf)
    opts = dict(optf(B, H), **({"gru_fence": 1} if fence else {}))
    tag = f"{case}{'+ragged' if ragged else ''}{'+fence' if fence else ''}[B{B},T{T},H{H}]"
    run = _forward(form, entry, dt, gi, w, b, opts, trace, nf)
    return run, _compare_forward(form, dt, tag, run, gi, w, b, nf)


# ---- forward ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form,dt", FORM_DT)
def test_forward_every_hidden_size(form, dt):
    _, _, _, hs, bh, _, _ = FORMS[form]
    bad = []
    for H in hs:
        bad += _one(form, dt, "gauss", bh, T0, H)[1]
    assert not bad, bad


@pytest.mark.parametrize("form,dt", FORM_DT)
def test_forward_every_batch_boundary(form, dt):
    """B = 17 and 33 leave one clip alone in the last 16-clip group, with 15 absent rows."""
    _, _, _, hs, _, bs, _ = FORMS[form]
    bad = []
    for B in bs:
        bad += _one(form, dt, "gauss", B, T0, hs[0])[1]
    assert not bad, bad


@pytest.mark.parametrize("form,dt", FORM_DT)
def test_forward_short_sequences(form, dt):
    _, _, _, hs, bh, _, _ = FORMS[form]
    bad = []
    for T in (1, 2, 3):
        bad += _one(form, dt, "gauss", bh, T, hs[0])[1]
    assert not bad, bad


@pytest.mark.parametrize("form,dt", FORM_DT)
def test_forward_input_cases(form, dt):
    """Trained-scale weights, saturated gates (+-30, +-1e4, +-inf: the limits 0, 1, +-1 exactly, no NaN; a +1e4 gi_z passes the carry
    through), a fully saturated z; for the f16x2 forms also a zero row and column of W_hh and columns spanning 2^-20 .. 2^3."""
    _, _, _, hs, bh, _, trace = FORMS[form]
    bad = []
    for case in ("trained", "sat", "all_sat") + (("zero_rowcol", "wide_cols") if trace[0] == "x2" else ()):
        run, b_ = _one(form, dt, case, bh, T0, hs[0])
        bad += b_
        if case == "all_sat":
            assert bool((run.out == 0).all()), "z = 1 from h = 0 must stay at 0 exactly"
        if case == "sat":
            h = run.out.reshape(bh, T0, 2, hs[0]).float()
            assert torch.equal(h[:, 2:T0 - 2, 0, 32:36], h[:, 1:2, 0, 32:36].expand(-1, T0 - 4, -1)), "z = 1 must pass h through"
            if run.gates is not None:
                r, z, n = (run.gates[..., i * hs[0]:(i + 1) * hs[0]] for i in range(3))
                assert bool((r[..., 24:28] == 1).all()) and bool((r[..., 28:32] == 0).all()) and bool((r[..., 44:48] == 1).all()) and bool((r[..., 48:52] == 0).all())
                assert bool((z[..., 52:56] == 0).all()) and bool((n[..., 56:60] == 1).all()) and bool((n[..., 60:64] == -1).all())
    assert not bad, bad


@pytest.mark.parametrize("form,dt", [(f, d) for f, d in FORM_DT if f not in ("F3", "F4")])
def test_forward_ragged(form, dt):
    """Lengths {T, 1, 2, T - 1, ...}, NaN in gi past each clip's end; rows t < n_frames[b] against the driven restatement (which reads
    h = 0 past the end, where the reverse direction starts; the rows there are unspecified and not looked at)."""
    _, _, _, hs, bh, _, _ = FORMS[form]
    bad = []
    for B in ((4, 6) if form == "F1" else (max(bh, 6) + (1 if bh == 17 else 0),)):
        bad += _one(form, dt, "gauss", B, T0, hs[0], ragged=True)[1]
    assert not bad, bad


@pytest.mark.parametrize("form,dt", [(f, d) for f, d in FORM_DT if f in ("F1", "F5", "F6")])
def test_forward_fence_variant(form, dt):
    """Option gru_fence = 1 (release / acquire instead of write-through): same traces, so pinned by the option; the same bits."""
    _, _, _, hs, bh, _, _ = FORMS[form]
    bad = []
    for B, ragged in ((bh, False), (17, False), (6, True)):
        run, b_ = _one(form, dt, "gauss", B, T0, hs[0], fence=True, ragged=ragged)
        plain, _ = _one(form, dt, "gauss", B, T0, hs[0], ragged=ragged)
        bad += b_
        nf = G.ragged_lengths(B, T0) if ragged else torch.full((B,), T0)
        for bb, n in enumerate(nf.tolist()):
            assert torch.equal(_bits(run.out[bb, :n]), _bits(plain.out[bb, :n])) and torch.equal(_bits(run.mish[bb, :n]), _bits(plain.mish[bb, :n]))
    assert not bad, bad


@pytest.mark.parametrize("form,dt", FORM_DT)
def test_forward_clips_do_not_see_each_other(form, dt):
    """The same call with every other clip's gi replaced by NaN and +-1e30: the watched clip's bits do not change (clip 0 and the last
    clip, which at B = 17 sits alone in its group beside 15 absent rows)."""
    entry, _, optf, hs, bh, _, trace = FORMS[form]
    H = hs[0]
    for B in sorted({bh, 17}):
        gi, w, b = G.forward_case("gauss", B, T0, H, dt)
        base = _forward(form, entry, dt, gi, w, b, optf(B, H), trace)
        for watched in (0, B - 1):
            other = _forward(form, entry, dt, G.foreign_clips(gi, watched), w, b, optf(B, H), trace)
            for a, c in ((base.out, other.out), (base.mish, other.mish), (base.gates, other.gates)):
                if a is not None:
                    assert torch.equal(_bits(a[watched]), _bits(c[watched])), (form, B, watched)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("B", [5, 17])
@pytest.mark.parametrize("H", [128, 256])
def test_16_bit_forms_give_the_same_bits(dt, B, H):
    """Four waves, eight waves with counters, granules, and the fence variants of the first two."""
    gi, w, b = G.forward_case("gauss", B, T0, H, dt)
    runs = []
    for form, opts in (("F5", {"gru_nw": 4}), ("F6", {"gru_handoff": 1}), ("F7", {"gru_handoff": 2}), ("F5", {"gru_nw": 4, "gru_fence": 1}),
                       ("F6", {"gru_handoff": 1, "gru_fence": 1})):
        runs.append(_forward(form, "layer", dt, gi, w, b, opts, FORMS[form][6]))
    for r in runs[1:]:
        assert torch.equal(_bits(r.out), _bits(runs[0].out)) and torch.equal(_bits(r.mish), _bits(runs[0].mish))


@pytest.mark.parametrize("form,dt", [("F2", "f32"), ("F3", "f32"), ("F7", "bf16"), ("F7", "f16")])
def test_granule_forms_are_deterministic(form, dt):
    entry, _, optf, hs, bh, _, trace = FORMS[form]
    B, H = 17, hs[1]
    gi, w, b = G.forward_case("gauss", B, T0, H, dt)
    a, c = (_forward(form, entry, dt, gi, w, b, optf(B, H), trace) for _ in range(2))
    for x, y in ((a.out, c.out), (a.mish, c.mish), (a.gates, c.gates)):
        if x is not None:
            assert torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize("form", ["F1", "F2", "F3", "F4"])
@pytest.mark.parametrize("H", [64, 320])
def test_float32_forms_free_running_against_nn_gru(form, H):
    """What a user sees: the whole sequence against float64 torch.nn.GRU fed the same gi, T = 37; bound 8 x E32, E32 = float32
    torch.nn.GRU on the CPU against the same float64 run.  Pins the restatement's formulas to torch on the device side as well."""
    entry, _, optf, _, bh, _, trace = FORMS[form]
    gi, w, b = G.forward_case("gauss", bh, T0, H)
    with torch.no_grad():
        r64, r32 = G.torch_gru(gi, w, b)[0], G.torch_gru(gi, w, b, torch.float32)[0]
    run = _forward(form, entry, "f32", gi, w, b, optf(bh, H), trace)
    for k, got, ref, y in (("h", run.out, r64, r32),) + ((("mish", run.mish, torch.nn.functional.mish(r64), torch.nn.functional.mish(r32)),) if run.mish is not None else ()):
        err, e32 = float((got.double() - ref).abs().max()), float((y.double() - ref).abs().max())
        print(f"{form}/f32 free-running[B{bh},T{T0},H{H}]:{k} {err:.3e} {e32:.3e} {err / e32:.2f}")
        assert err <= FACTOR * e32, (form, H, k, err, e32)


# ---- backward -----------------------------------------------------------------------------------------------------------------------

def _bwd_trace(form):
    return ("bwd_x2", 64) if form == "B1" else ("bwd_counter", 32)


def _bwd_one(form, case, B, T, H):
    optf = BWD[form][0]
    gates, out, dout, w = G.backward_case(case, B, T, H)
    got = _backward(form, gates, out, dout, w, optf(B, H), _bwd_trace(form))
    return got, _compare_backward(form, f"{case}[B{B},T{T},H{H}]", got, gates, out, dout, w)


@pytest.mark.parametrize("form", ["B1", "B2"])
def test_backward_every_hidden_size(form):
    """B1: gru_bwd_x2_kernel<1> .. <6>."""
    bad = []
    for H in H64:
        bad += _bwd_one(form, "gauss", BWD[form][1], T0, H)[1]
    assert not bad, bad


@pytest.mark.parametrize("form", ["B1", "B2"])
def test_backward_every_batch_boundary_and_short_sequences(form):
    bad = []
    for B in BWD[form][2]:
        bad += _bwd_one(form, "gauss", B, T0, 128)[1]
    for T in (1, 2, 3):
        for H in (64, 128):
            bad += _bwd_one(form, "gauss", BWD[form][1], T, H)[1]
    assert not bad, bad


@pytest.mark.parametrize("form", ["B1", "B2"])
def test_backward_input_cases(form):
    """Trained-scale weights, a zero row and column of W_hh, columns spanning 2^-20 .. 2^3, one clip without gradient beside one with
    1e6 times the others', and no gradient at all (exact zeros)."""
    bad = []
    for case in G.BWD_CASES[1:]:
        got, b_ = _bwd_one(form, case, BWD[form][1], T0, 128)
        bad += b_
        if case == "dout_zero":
            assert bool((got[0] == 0).all()) and bool((got[1] == 0).all())
        if case == "clip_scales":
            assert bool((got[0][0] == 0).all()) and bool((got[1][0] == 0).all()), "a clip without gradient must stay at zero beside a large one"
    assert not bad, bad


@pytest.mark.parametrize("form", ["B1", "B2"])
def test_backward_clips_do_not_see_each_other(form):
    optf, bh, _ = BWD[form]
    H = 128
    for B in (bh, 17):
        gates, out, dout, w = G.backward_case("gauss", B, T0, H)
        base = _backward(form, gates, out, dout, w, optf(B, H), _bwd_trace(form))
        for watched in (0, B - 1):
            other = _backward(form, G.foreign_clips(gates, watched), G.foreign_clips(out, watched, 1), G.foreign_clips(dout, watched, 2), w,
                              optf(B, H), _bwd_trace(form))
            for a, c in zip(base, other):
                assert torch.equal(_bits(a[watched]), _bits(c[watched])), (form, B, watched)


def test_backward_x2_is_deterministic():
    gates, out, dout, w = G.backward_case("gauss", 17, T0, 256)
    a, c = (_backward("B1", gates, out, dout, w, {}, _bwd_trace("B1")) for _ in range(2))
    assert torch.equal(_bits(a[0]), _bits(c[0])) and torch.equal(_bits(a[1]), _bits(c[1]))
