"""The emission head kernels (csrc/la_head.hip: la_fc_emissions, la_fc_emissions_x2; csrc/la_elementwise.hip: la_emissions_from_logits)
against the float64 restatement of tests/head_reference.py, through the C ABI, at the smallest shapes that select each kernel form.

Set-up of every call: `em` is a pitched view (row stride max_labels + 4, batch stride frames * row stride + 11) inside a sentinel-filled
Guard, and the columns past 1 + min(n_labels, max_labels) of each clip must keep the sentinel; `act` is pitched (K + 16 elements for
16-bit types, K + 4 for float32, the pad columns hold 50); labels_stride is max_labels + 2; the workspace is exactly the queried size,
256-byte aligned, with sentinel bytes on both sides.  The clips of a batch are drawn in rotation from six kinds -- n_labels 0, 1,
max_labels, max_labels + 3 (clamped), a repeated label, class ids 0, -1, hi + 1 and V (exactly -1000) -- so a form with fewer than six
clips per call meets every kind over its cases.

Which form ran is observed, not read off the source: the launch count of the kernel timer family (fc_lse_bf16 / fc_lse_f32) and the
number of 64-column strips per row the call left in the workspace (the 256-column kernels write 4 ceil(V / 256) strips, the 128-column
kernels 2 ceil(V / 128): 256 against 254 at V = 16130).  The hand-placed and the ping-pong loop of the 256 x 256 kernel and the 128- and
256-row tile of the 128-column kernel differ in neither, so those are pinned by their option and must give the same bits.

Measured group: ref = the restatement in float64 on the dtype-rounded operands, E32 = the error of the same restatement evaluated by
torch on the CPU in float32 on the same operands (16-bit operands converted to float32 first), gate rel_err(got, ref) <= 8 x E32 with the
metric and factor of tests/test_gpu_row_kernels.py; every comparison prints `kernel case err E32 ratio`, the lines of one MI355X run are
kept in profiles/head_kernel_errors.txt.  In every fused case row V - 1 of w_fc is the unit vector e_0 and b_fc[V - 1] is 0 (CTC), so the
silence logit of row r is act[r][0] exactly in every kernel; measured cases keep it on linspace(-2, 2) rounded to 1/8.
Decisive group: biases that make an excluded, a dropped or a padding column move every emission by 0.5 or more, bound 1e-2.
Silence sweep: the logits of head_reference.sweep_values() -- em[..][0] exactly -1000 at x0 <= -89, inside silence_bracket(x0) otherwise;
label columns inside [lsm64 + v_lo, lsm64 + v_hi] (each end clamped at -1000) widened by 8 x E32_lsm, which is the issue's "within
8 x E32_lsm plus the bracket's half-width" read about the bracket (the float64 value itself lies outside it from x0 = 16.75 on, where
float32 has 1 - sil = 0), and exactly -1000 where every bracket candidate saturates; la_emissions_from_logits on the materialised
float32 logits of the same case must give em[..][0] bit for bit.
"""
import ctypes
import functools
import math

import pytest
import torch

import head_reference as H
from test_gpu_row_kernels import FACTOR, Guard, _bits, _dev, _g, _L, _measured, _ok, _st

pytestmark = pytest.mark.gpu

DT = {"f32": (torch.float32, 0, 4), "bf16": (torch.bfloat16, 1, 2), "f16": (torch.float16, 2, 2)}
WS_SENT = 0x5A
LMAX = 7
KINDS = ("n0", "n1", "nmax", "clamped", "repeat", "bad_ids")


class _count_launches:
    """Launches of one kernel family (la_timer_*, exact name) inside the block."""

    def __init__(self, family):
        self.family, self.n = family, 0

    def __enter__(self):
        L = _L()
        L.la_timer_reset(); L.la_timer_sample(1000003); L.la_timer_enable(self.family.encode())
        return self

    def __exit__(self, *exc):
        L = _L()
        torch.cuda.synchronize()
        L.la_timer_disable()
        ms, timed, work, seen = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_double(0), ctypes.c_int64(0)
        L.la_timer_read_work(ctypes.byref(ms), ctypes.byref(timed), ctypes.byref(work), ctypes.byref(seen))
        self.n = int(seen.value)
        L.la_timer_reset(); L.la_timer_sample(1)
        return False


# ---- operands -----------------------------------------------------------------------------------------------------------------------

def _grid(rows):
    return torch.round(torch.linspace(-2.0, 2.0, rows) * 8) / 8


def _silence(rows, kind):
    """act[:, 0] = the silence logit of every row: 'grid' (measured cases), 'plus8' (decisive CTC), 'sweep'."""
    if kind == "grid":
        return _grid(rows)
    if kind == "plus8":
        return torch.full((rows,), 8.0)
    xs = H.sweep_values()
    assert rows >= xs.numel(), (rows, xs.numel())
    return xs[torch.arange(rows) % xs.numel()]


@functools.lru_cache(maxsize=2)
def _base(dt, rows, K, V):
    """act ~ N(0, 1), w ~ N(0, (2 / sqrt K)^2), bias ~ N(0, 0.5^2) as in test_fc_emissions_fused, rounded to the dtype; row V - 1 of w is
    e_0 and its bias 0.  One draw per (dtype, shape): every case of a form shares it."""
    dtype = DT[dt][0]
    g = _g(rows * 31 + K * 7 + V)
    act = torch.randn(rows, K, generator=g).to(dtype)
    w = (torch.randn(V, K, generator=g) * (2.0 / K ** 0.5)).to(dtype)
    bias = torch.randn(V, generator=g) * 0.5
    w[V - 1] = 0
    w[V - 1, 0] = 1
    bias[V - 1] = 0
    return act, w, bias


@functools.lru_cache(maxsize=3)
def _products(dt, rows, K, V, kind, zero_rows=()):
    """(act, w) in the dtype with act[:, 0] = the silence logits of `kind`, and act @ w.T in float64 and in float32 (no bias: the cases of
    one form differ in their biases and share the product).  zero_rows: rows of w set to zero (the clamp case)."""
    act, w, _ = _base(dt, rows, K, V)
    act, w = act.clone(), w.clone()
    act[:, 0] = _silence(rows, kind).to(act.dtype)
    for c in zero_rows:
        w[c] = 0
    return act, w, act.double() @ w.double().T, act.float() @ w.float().T


def _labels(B, V, variant, case_index, force=()):
    """[B][LMAX + 2] int32 labels and [B] n_labels: clip b of case i is of kind KINDS[(i B + b) % 6].  force: class ids placed at the
    first label positions of every clip (those with fewer labels drop them)."""
    _, hi = H.norm_range(V, variant)
    g = _g(1000 + case_index * 17 + V)
    lab = torch.randint(1, hi + 1, (B, LMAX + 2), generator=g, dtype=torch.int32)
    n = torch.zeros(B, dtype=torch.int32)
    kinds = []
    for b in range(B):
        kind = KINDS[(case_index * B + b) % len(KINDS)]
        kinds.append(kind)
        n[b] = {"n0": 0, "n1": 1, "nmax": LMAX, "clamped": LMAX + 3, "repeat": LMAX, "bad_ids": LMAX}[kind]
        for i, c in enumerate(force):
            lab[b, i] = c
        if kind == "repeat":
            lab[b, 4] = lab[b, 3]
        if kind == "bad_ids":
            lab[b, 3:7] = torch.tensor([0, -1, hi + 1, V], dtype=torch.int32)
    return lab, n, kinds


# ---- one call -----------------------------------------------------------------------------------------------------------------------

class _Workspace:
    """Exactly `need` bytes at a 256-byte boundary, sentinel bytes before and after."""

    def __init__(self, need):
        self.need = need
        self.buf = torch.full((need + 1024,), WS_SENT, dtype=torch.uint8, device="cuda")
        self.off = (-self.buf.data_ptr()) % 256 + 256
        self.ptr = self.buf.data_ptr() + self.off
        assert self.ptr % 256 == 0

    def check(self):
        torch.cuda.synchronize()
        host = self.buf.cpu()
        assert bool((host[: self.off] == WS_SENT).all()) and bool((host[self.off + self.need:] == WS_SENT).all()), "written outside the workspace"
        return host[self.off: self.off + self.need]


def _strips_written(ws_bytes, layout, rows):
    """64-column strips per row that the call wrote into the partials part of the workspace (8 bytes each, filled front to back)."""
    off, n = layout["partials"]
    words = ws_bytes[off: off + n].contiguous().view(torch.int32)
    touched = int((words != 0x5A5A5A5A).sum())
    assert touched % (2 * rows) == 0 and bool((words[:touched] != 0x5A5A5A5A).all()), "partials are not one dense [rows][strips] block"
    return touched // (2 * rows)


def _fc(dt, B, T, K, V, variant, act, w, bias, lab, n_lab, x2=False):
    """One call of la_fc_emissions / la_fc_emissions_x2 in the common set-up -> (em [B][T][1 + LMAX] on the host, strips per row)."""
    L = _L()
    dtype, code, es = DT[dt]
    rows = B * T
    ld = K + (4 if dt == "f32" else 16)
    actp = torch.full((rows, ld), 50.0, dtype=dtype)
    actp[:, :K] = act
    actd, wd, bd, labd, nd = _dev(actp), _dev(w), _dev(bias.float()), _dev(lab), _dev(n_lab)
    rs = LMAX + 4
    em = Guard((B, T, 1 + LMAX), (T * rs + 11, rs, 1))
    need = ctypes.c_size_t(0)
    if x2:
        planes = torch.empty((V, 2, K), dtype=torch.float16, device="cuda")
        inv = torch.empty((V,), dtype=torch.float32, device="cuda")
        _ok(L.la_split_f16x2(wd.data_ptr(), K, V, K, planes.data_ptr(), K, inv.data_ptr(), _st()), "split_f16x2")
        _ok(L.la_fc_emissions_x2_workspace_bytes(B, T, K, V, LMAX, ctypes.byref(need)), "x2 workspace query")
        ws = _Workspace(need.value)
        _ok(L.la_fc_emissions_x2(actd.data_ptr(), ld, wd.data_ptr(), bd.data_ptr(), planes.data_ptr(), inv.data_ptr(), B, T, K, V, variant,
                                 labd.data_ptr(), LMAX + 2, nd.data_ptr(), LMAX, em.ptr, T * rs + 11, rs, ws.ptr, need.value, _st()), "fc_emissions_x2")
    else:
        _ok(L.la_fc_emissions_workspace_bytes(code, B, T, K, V, LMAX, ctypes.byref(need)), "workspace query")
        ws = _Workspace(need.value)
        _ok(L.la_fc_emissions(code, actd.data_ptr(), ld, wd.data_ptr(), bd.data_ptr(), B, T, K, V, variant, labd.data_ptr(), LMAX + 2,
                              nd.data_ptr(), LMAX, em.ptr, T * rs + 11, rs, ws.ptr, need.value, _st()), "fc_emissions")
    em.check()
    layout = H.workspace_layout(B, T, K, V, LMAX, es, x2 and H.x2_domain(rows, K, V))
    assert layout["total"] == need.value
    strips = _strips_written(ws.check(), layout, rows)
    return em.get(), strips


def _from_logits(lg, variant, lab, n_lab, max_labels, pitch=5):
    """la_emissions_from_logits on float32 logits [B][T][V] with a pitched row stride -> em on the host."""
    L = _L()
    B, T, V = lg.shape
    rsl = V + pitch
    lp = torch.full((B, T, rsl), 1e30)                 # pad columns above every logit: they must not be read
    lp[..., :V] = lg
    lgd, labd, nd = _dev(lp), _dev(lab), _dev(n_lab)
    rs = max_labels + 4
    em = Guard((B, T, 1 + max_labels), (T * rs + 11, rs, 1))
    _ok(L.la_emissions_from_logits(lgd.data_ptr(), T * rsl, rsl, B, T, V, variant, labd.data_ptr(), lab.shape[1], nd.data_ptr(), max_labels,
                                   em.ptr, T * rs + 11, rs, _st()), "emissions_from_logits")
    em.check()
    return em.get()


def _check_layout(got, ref, n_lab, kinds, max_labels=LMAX):
    """Unwritten columns keep the sentinel, written ones hold no sentinel-like leftovers; invalid class ids are exactly -1000; a
    repeated label gives identical columns.  -> the mask of written entries."""
    wr = H.written(n_lab, max_labels).unsqueeze(1).expand_as(got)
    assert bool((got[~wr] == 7.0).all()), "a column past 1 + min(n_labels, max_labels) was written"
    assert torch.equal(torch.isnan(ref), ~wr)
    assert bool(torch.isfinite(got[wr]).all()) and bool((got[wr] >= -1000.0).all())
    for b, kind in enumerate(kinds):
        if kind == "bad_ids":
            assert bool((got[b, :, 4:8] == -1000.0).all()), "an out-of-range class id did not give -1000"
        if kind == "repeat":
            assert torch.equal(got[b, :, 4], got[b, :, 5])
    return wr


# ---- the cases of one form ----------------------------------------------------------------------------------------------------------

def _reference(P64, P32, bias, B, T, variant):
    lg64 = (P64 + bias.double()).reshape(B, T, -1)
    lg32 = (P32 + bias.float()).reshape(B, T, -1)
    return lg64, H.parts(lg64, variant), H.parts(lg32, variant)


def _spike_column(V):
    """The middle of a 64-column strip, inside both normaliser ranges."""
    return 64 * ((V // 64) // 2) + 32 if V > 96 else min(32, V - 2)


# the label set of a case depends on its name alone, so two forms that must give the same bits see the same call
CASE_INDEX = {(tag, v): 2 * i + v for i, tag in enumerate(("gauss", "bias+100", "act*8", "spike+30", "decisive+8", "decisive", "clamp")) for v in (0, 1)}
_REFS = {}        # (dtype, B, T, rows of the operands, K, V, case, variant) -> (ref, e32) in the compact layout: small


def _run_form(name, dt, B, T, K, V, *, x2=False, family=None, strips=None, extras=True, only=None, rows_from=None):
    """Every case of one kernel form at one shape (extras=False: the Gaussian and the decisive cases; only: those tags).
    rows_from = (B', T'): the operands are the first B T rows of that larger shape's (the 512-row run on the 513-row operands).
    Returns {case: em} for bit comparisons between forms."""
    rows = B * T
    src_rows = rows if rows_from is None else rows_from[0] * rows_from[1]
    out = {}
    _, _, bias0 = _base(dt, src_rows, K, V)

    def case(tag, variant, kind, bias, *, decisive=False, measured=True, zero_rows=(), force=(), act_scale=1.0, count=False):
        if only is not None and tag not in only:
            return None
        act, w, P64, P32 = _products(dt, src_rows, K, V, kind, zero_rows)
        act = act[:rows] * act_scale                                   # a power of two: exact in every format, and in the products
        lab, n_lab, kinds = _labels(B, V, variant, CASE_INDEX[(tag, variant)], force)
        if count:
            with _count_launches(family) as c:
                got, st = _fc(dt, B, T, K, V, variant, act, w, bias, lab, n_lab, x2)
            assert c.n == 1, (name, family, c.n)
            with _count_launches("fc_lse_f32" if family == "fc_lse_bf16" else "fc_lse_bf16") as c:
                got2, _ = _fc(dt, B, T, K, V, variant, act, w, bias, lab, n_lab, x2)
            assert c.n == 0 and torch.equal(_bits(got2), _bits(got))
        else:
            got, st = _fc(dt, B, T, K, V, variant, act, w, bias, lab, n_lab, x2)
        if strips is not None:
            assert st == strips, (name, tag, st, strips)
        key = (dt, B, T, src_rows, K, V, tag, variant)
        if key not in _REFS:
            _, p64, p32 = _reference(P64[:rows] * act_scale, P32[:rows] * act_scale, bias, B, T, variant)
            _REFS[key] = H.compact(*p64, lab, n_lab, LMAX, variant), H.compact(*p32, lab, n_lab, LMAX, variant)
        ref, e32 = _REFS[key]
        wr = _check_layout(got, ref, n_lab, kinds)
        label = f"{dt},B={B},T={T},K={K},V={V},{'ctc' if variant else 'plain'},{tag}"
        if decisive:
            err = float((got[wr].double() - ref[wr]).abs().max())
            print(f"{name} {label} max|err| {err:.3e} bound=1e-2")
            assert err < 1e-2, (name, label, err)
        if measured:
            _measured(name, label, got[wr], ref[wr], e32[wr])
        out[(tag, variant)] = got
        return got, n_lab

    # measured: both variants on the plain operands (the first call also shows which timer family launched)
    case("gauss", H.CTC, "grid", bias0, count=family is not None)
    case("gauss", H.PLAIN, "grid", bias0)
    if extras:
        b100 = bias0 + 100.0
        case("bias+100", H.PLAIN, "grid", b100)
        b100 = b100.clone()
        b100[V - 1] = 0.0                                              # the silence logit stays act[r][0]
        case("bias+100", H.CTC, "grid", b100)
        case("act*8", H.PLAIN, "grid", bias0, act_scale=8.0)           # plain: a CTC silence logit of 16 would only measure log(1 - sil)
        if V >= 65:
            bs = bias0.clone()
            bs[_spike_column(V)] += 30.0
            case("spike+30", H.PLAIN, "grid", bs)
            case("spike+30", H.CTC, "grid", bs)
    # decisive: CTC column 0 at +40 (excluded, never a label) and the silence logit at +8 (column V - 1 excluded), then the same biases
    # on the bounded grid under the measured gate; plain columns 0 and V - 1 at +10 (included; padding columns read bias[V - 1])
    bd = bias0.clone()
    bd[0] = 40.0
    case("decisive+8", H.CTC, "plus8", bd, decisive=True, measured=False)
    case("decisive", H.CTC, "grid", bd, decisive=True)
    bd = bias0.clone()
    bd[0], bd[V - 1] = 10.0, 10.0
    case("decisive", H.PLAIN, "grid", bd, decisive=True)
    # clamp: class c1 sits at exactly -2000 (zero weight row), class c2 at -900 + w . a
    if V >= 65 and extras:
        c1, c2 = 5, 37
        bc = bias0.clone()
        bc[c1], bc[c2] = -2000.0, -900.0
        for variant in (H.CTC, H.PLAIN):
            res = case("clamp", variant, "grid", bc, zero_rows=(c1,), force=(c1, c2))
            if res is not None:
                got, n_lab = res
                for b in range(B):
                    if int(n_lab[b]) >= 2:
                        assert bool((got[b, :, 1] == -1000.0).all()) and bool((got[b, :, 2] > -1000.0).all()) and bool((got[b, :, 2] < -850.0).all())
    return out


@functools.lru_cache(maxsize=None)
def _bracket(x0):
    return H.silence_bracket(x0)


def _run_sweep(name, dt, B, T, K, V, x2=False, strips=None):
    """The silence sweep of one form (CTC), and la_emissions_from_logits on the same logits rounded to float32."""
    rows = B * T
    act, w, P64, P32 = _products(dt, rows, K, V, "sweep")
    _, _, bias = _base(dt, rows, K, V)
    lab, n_lab, kinds = _labels(B, V, H.CTC, 3)
    got, st = _fc(dt, B, T, K, V, H.CTC, act, w, bias, lab, n_lab, x2)
    if strips is not None:
        assert st == strips
    lg64 = (P64 + bias.double()).reshape(B, T, V)
    x0 = _silence(rows, "sweep").reshape(B, T)
    assert torch.equal(lg64[..., V - 1], x0.double()), "the silence logit is not exact in the reference"
    lsm64 = H.log_softmax_part(lg64, H.CTC)
    e32_lsm = H.rel_err(H.log_softmax_part((P32 + bias.float()).reshape(B, T, V), H.CTC)[..., 1:V - 1], lsm64[..., 1:V - 1])
    lg32 = lg64.float()
    assert torch.equal(lg32[..., V - 1], x0)
    got_fl = _from_logits(lg32, H.CTC, lab, n_lab, LMAX)
    lsm64_fl = H.log_softmax_part(lg32.double(), H.CTC)
    e32_fl = H.rel_err(H.log_softmax_part(lg32, H.CTC)[..., 1:V - 1], lsm64_fl[..., 1:V - 1])
    br = [_bracket(float(v)) for v in x0.reshape(-1).tolist()]
    col = lambda f: torch.tensor([f(x) for x in br], dtype=torch.float64).reshape(B, T)
    s_lo, s_hi, v_lo, v_hi = col(lambda x: x[0][0]), col(lambda x: x[0][1]), col(lambda x: x[1][0]), col(lambda x: x[1][1])
    sat = torch.tensor([x[2] for x in br]).reshape(B, T)
    dead = x0 <= -89.0
    assert int(dead.sum()) >= 16 and int((x0 >= 16.75).sum()) >= 20
    for who, em, lsm, e32 in ((name, got, lsm64, e32_lsm), ("la_emissions_from_logits", got_fl, lsm64_fl, e32_fl)):
        wr = H.written(n_lab, LMAX).unsqueeze(1).expand_as(em)
        assert bool((em[~wr] == 7.0).all()) and bool(torch.isfinite(em[wr]).all()) and bool((em[wr] >= -1000.0).all())
        e0 = em[..., 0].double()
        assert bool((e0[dead] == -1000.0).all()), (who, "log sil at x0 <= -89")
        inside = (e0 >= s_lo) & (e0 <= s_hi)
        assert bool(inside[~dead].all()), (who, x0[~dead & ~inside].tolist(), e0[~dead & ~inside].tolist())
        worst = 0.0
        for b in range(B):
            Lb = min(int(n_lab[b]), LMAX)
            cls = lab[b, :Lb].long()
            valid = (cls >= 1) & (cls <= V - 2)
            e = em[b, :, 1:1 + Lb].double()
            assert bool((e[:, ~valid] == -1000.0).all())
            if not bool(valid.any()):
                continue
            e, l64 = e[:, valid], lsm[b][:, cls[valid]]
            assert bool((e[sat[b]] == -1000.0).all()), (who, "label columns where 1 - sil is 0 for every candidate")
            tol = FACTOR * e32 * l64.abs().clamp_min(1.0)
            lo = (l64 + v_lo[b].unsqueeze(1)).clamp_min(-1000.0) - tol
            hi = (l64 + v_hi[b].unsqueeze(1)).clamp_min(-1000.0) + tol
            ok = ((e >= lo) & (e <= hi)) | sat[b].unsqueeze(1)
            assert bool(ok.all()), (who, b, x0[b][~ok.all(1)].tolist())
            narrow = (hi - lo) < 1.0                                       # where the bracket is a few ulps wide: the position inside it
            if bool(narrow.any()):
                worst = max(worst, float((((e - 0.5 * (lo + hi)).abs() / (0.5 * (hi - lo)))[narrow]).max()))
        print(f"{who} {dt},B={B},T={T},K={K},V={V},ctc,sweep e32_lsm={e32:.3e} label columns at most {worst:.2f} of the way to the bracket's edge")
    same = torch.equal(_bits(got[..., 0].contiguous()), _bits(got_fl[..., 0].contiguous()))
    print(f"{name} {dt},B={B},T={T},K={K},V={V},ctc,sweep em[..][0] equals la_emissions_from_logits bit for bit: {same}")
    assert same, "the fused merge and la_emissions_from_logits evaluate the silence term differently"


# ---- the 128-column kernels at small shapes -----------------------------------------------------------------------------------------
# Fewer than 192 tiles of 256 x 256 (pp_ok and fc_x2_ok false) and gemm_tile unset: the 128-row form of route_lse,
# fc_lse_kernel<float, Small> for float32 and fc_lse_kernel<T16, Small> for bf16 / f16.

@pytest.mark.parametrize("B,T,K,V", [(5, 1, 32, 3), (5, 1, 32, 65), (3, 43, 32, 129), (3, 43, 96, 65), (3, 43, 96, 300), (5, 1, 96, 129)])
def test_float32_small_kernel(B, T, K, V):
    """V = 3 is the smallest CTC vocabulary (one normalised column); plain at its smallest, V = 2, runs beside it."""
    st = 2 * -(-V // 128) if 2 * -(-V // 128) != 4 * -(-V // 256) else None
    _run_form("fc_lse_kernel<float,Small>", "f32", B, T, K, V, family="fc_lse_f32", strips=st)
    if V == 3:
        rows = B * T
        act, w, bias = _base("f32", rows, K, 2)
        act = act.clone()
        act[:, 0] = _grid(rows)
        for i, b in enumerate((bias, bias + 100.0, torch.tensor([10.0, 10.0]))):
            lab, n_lab, kinds = _labels(B, 2, H.PLAIN, i)
            got, _ = _fc("f32", B, T, K, 2, H.PLAIN, act, w, b, lab, n_lab)
            p64 = H.parts((act.double() @ w.double().T + b.double()).reshape(B, T, 2), H.PLAIN)
            p32 = H.parts((act @ w.T + b).reshape(B, T, 2), H.PLAIN)
            ref, e32 = H.compact(*p64, lab, n_lab, LMAX, H.PLAIN), H.compact(*p32, lab, n_lab, LMAX, H.PLAIN)
            wr = _check_layout(got, ref, n_lab, kinds)
            assert float((got[wr].double() - ref[wr]).abs().max()) < 1e-2
            _measured("fc_lse_kernel<float,Small>", f"f32,B={B},T={T},K={K},V=2,plain,case{i}", got[wr], ref[wr], e32[wr])


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("K,V", [(64, 65), (64, 300), (192, 129), (192, 300)])
def test_16bit_small_kernel(dt, K, V):
    st = 2 * -(-V // 128) if 2 * -(-V // 128) != 4 * -(-V // 256) else None
    _run_form(f"fc_lse_kernel<{dt},Small>", dt, 3, 43, K, V, family="fc_lse_bf16", strips=st)


@pytest.mark.parametrize("dt,K", [("f32", 32), ("bf16", 64), ("f16", 64)])
def test_small_kernel_silence_sweep(dt, K):
    """3 x 112 = 336 rows, one per sweep value."""
    assert H.sweep_values().numel() == 336
    _run_sweep(f"fc_lse_kernel<{dt},Small>", dt, 3, 112, K, 65)


# ---- the 256 x 256 kernels --------------------------------------------------------------------------------------------------------
# 513 rows x 16130 columns = 3 x 64 = 192 tiles of 256 x 256, exactly the threshold of pp_ok / fc_x2_ok, with 1 row in the last row
# tile and 2 columns in the last column tile.  K = 128: not a multiple of 128 from 256 on, so the ping-pong loop (fc_lse_pp_kernel<T16>);
# K = 256: the hand-placed loop (fc_lse_pp_kernel<T16, true>), and with option gemm_loop = 99 the ping-pong loop again.  512 rows are
# 2 x 64 = 128 tiles: the Small kernel on the same operands.

BIG = (3, 171, 16130)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("K", [128, 256])
def test_16bit_256x256_kernel(dt, K):
    B, T, V = BIG
    form = f"fc_lse_pp_kernel<{dt}{',true' if K == 256 else ''}>"
    out = _run_form(form, dt, B, T, K, V, family="fc_lse_bf16", strips=256)
    if K == 256:
        from lyricalignment_amd import _lib
        with _lib.option("gemm_loop", 99):
            assert _lib.get_option("gemm_loop") == 99
            pp = _run_form(f"fc_lse_pp_kernel<{dt}>@K=256", dt, B, T, K, V, family="fc_lse_bf16", strips=256, extras=False)
        for key, em in pp.items():            # the header: the loop of the other K, identical bits
            assert torch.equal(_bits(em), _bits(out[key])), key
    _run_form(f"fc_lse_kernel<{dt},Small>@512rows", dt, 2, 256, K, V, family="fc_lse_bf16", strips=254, only=("gauss",), rows_from=(B, T))


@pytest.mark.parametrize("K", [128, 256])
def test_bf16_256x256_kernel_on_a_second_device(K):
    """The forms that need their dynamic-LDS ceiling raised (128 KiB), on a device other than 0: the ceiling is a per-device attribute of
    the kernel, so a process that has launched on device 0 must still raise it on device 1.  K = 128 the ping-pong loop, K = 256 the
    hand-placed loop; the Gaussian case under the usual layout, guard and error checks (the float64 references are the device-0 tests'),
    and the same bits as the same call on device 0."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second device")
    B, T, V = BIG
    form = f"fc_lse_pp_kernel<bf16{',true' if K == 256 else ''}>"
    first = _run_form(form, "bf16", B, T, K, V, family="fc_lse_bf16", strips=256, only=("gauss",))
    with torch.cuda.device(1):
        second = _run_form(form + "@device1", "bf16", B, T, K, V, family="fc_lse_bf16", strips=256, only=("gauss",))
        torch.cuda.synchronize()
    assert first.keys() == second.keys() and len(first) == 2
    for key, em in second.items():
        assert torch.equal(_bits(em), _bits(first[key])), key


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("K,loop", [(128, 0), (256, 0), (256, 99)])
def test_16bit_256x256_kernel_silence_sweep(dt, K, loop):
    from lyricalignment_amd import _lib
    B, T, V = BIG
    with _lib.option("gemm_loop", loop):
        _run_sweep(f"fc_lse_pp_kernel<{dt}{',true' if K == 256 and not loop else ''}>", dt, B, T, K, V, strips=256)


def test_bf16_256_row_tile_of_the_128_column_kernel():
    """Option gemm_tile = 256 switches pp_ok off; bf16 with 4096 rows or more then takes fc_lse_kernel<bf16_t, Big> (1 x 4097 rows: 17 row
    tiles, 1 row in the last).  Without the option the same call takes the Small kernel (17 x 2 tiles of 256 x 256 < 192), which
    accumulates in the same order: the same bits."""
    from lyricalignment_amd import _lib
    with _lib.option("gemm_tile", 256):
        assert _lib.get_option("gemm_tile") == 256
        big = _run_form("fc_lse_kernel<bf16,Big>", "bf16", 1, 4097, 64, 300, family="fc_lse_bf16", strips=6)
        _run_sweep("fc_lse_kernel<bf16,Big>", "bf16", 1, 4097, 64, 300, strips=6)
    small = _run_form("fc_lse_kernel<bf16,Small>@4097rows", "bf16", 1, 4097, 64, 300, family="fc_lse_bf16", strips=6, extras=False)
    for key, em in small.items():
        assert torch.equal(_bits(em), _bits(big[key])), key


def test_float32_normaliser_on_the_f16_pipe():
    """la_fc_emissions_x2 inside the 256 x 256 kernel's domain (K = 256, 192 tiles): fc_lse_x2_kernel."""
    B, T, V = BIG
    _run_form("fc_lse_x2_kernel", "f32", B, T, 256, V, x2=True, family="fc_lse_f32", strips=256)
    _run_sweep("fc_lse_x2_kernel", "f32", B, T, 256, V, x2=True, strips=256)


@pytest.mark.parametrize("K,V", [(128, 16130), (256, 300)])
def test_float32_x2_entry_outside_its_domain_takes_the_float32_kernel(K, V):
    """K = 128 is no multiple of 128 from 256 on; V = 300 gives 3 x 2 tiles: fc_x2_ok is false, the planes are ignored and the call must
    give the bits of la_fc_emissions on the same operands."""
    B, T = 3, 171
    st = 2 * -(-V // 128)
    x2 = _run_form("x2_entry->fc_lse_kernel<float,Small>", "f32", B, T, K, V, x2=True, family="fc_lse_f32", strips=st, extras=V == 300)
    plain = _run_form("fc_lse_kernel<float,Small>", "f32", B, T, K, V, family="fc_lse_f32", strips=st, extras=False)
    for key, em in plain.items():
        assert torch.equal(_bits(em), _bits(x2[key])), key
    if V == 300:
        _run_sweep("x2_entry->fc_lse_kernel<float,Small>", "f32", B, T, K, V, x2=True, strips=st)


# ---- la_emissions_from_logits -------------------------------------------------------------------------------------------------------

def _fl_labels(B, V, variant, max_labels, index):
    _, hi = H.norm_range(V, variant)
    g = _g(index * 13 + V)
    lab = torch.randint(1, hi + 1, (B, max_labels + 2), generator=g, dtype=torch.int32)
    n = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        kind = (index * B + b) % 4
        n[b] = (max_labels, max_labels + 3, 1, 0)[kind]
        if kind == 1:
            lab[b, 0:4] = torch.tensor([0, -1, hi + 1, V], dtype=torch.int32)
        lab[b, 4] = lab[b, 3]
    return lab, n


@pytest.mark.parametrize("variant", [H.CTC, H.PLAIN])
@pytest.mark.parametrize("B,T,V", [(2, 3, 3), (1, 37, 3), (2, 3, 257), (1, 37, 257), (2, 3, 513), (1, 37, 513), (2, 3, 21129), (1, 37, 21129)])
def test_emissions_from_logits(variant, B, T, V):
    """Exact float32 inputs on a 1/8 grid: Gaussian rows, the same + 1e4, rows with -inf in part of the normalised columns, a row with one
    finite normalised column (log-softmax exactly 0 there; CTC: silence logit -40, where 1 - sil is exactly 1 in float32 and in float64).  max_labels 7
    and 300 (the 256-thread label loop's second trip)."""
    lo, hi = H.norm_range(V, variant)
    g = _g(V * 3 + T)
    base = torch.round(torch.randn(B, T, V, generator=g) * 3 * 8) / 8
    if variant == H.CTC:
        base[..., V - 1] = _grid(B * T).reshape(B, T)
    for tag in ("gauss", "offset+1e4", "neg_inf"):
        lg = base.clone()
        if tag == "offset+1e4":
            lg[..., lo:hi + 1] += 1e4
        if tag == "neg_inf":
            if hi - lo >= 4:
                lg[:, :, lo + 1:hi + 1:3] = -math.inf          # a third of the normalised columns
            lg[0, 0, lo:hi + 1] = -math.inf
            one = lo + (hi - lo) // 2
            lg[0, 0, one] = 2.5                                # the only finite column of its row
            if variant == H.CTC:
                lg[0, 0, V - 1] = -40.0
        for max_labels in (7, 300):
            lab, n_lab = _fl_labels(B, V, variant, max_labels, max_labels + len(tag))
            if tag == "neg_inf" and hi > lo:
                lab[0, 0] = one
                lab[0, 1] = one + 1
            got = _from_logits(lg, variant, lab, n_lab, max_labels)
            ref, e32 = H.emissions(lg.double(), lab, n_lab, max_labels, variant), H.emissions(lg, lab, n_lab, max_labels, variant)
            wr = H.written(n_lab, max_labels).unsqueeze(1).expand_as(got)
            assert bool((got[~wr] == 7.0).all()) and torch.equal(torch.isnan(ref), ~wr)
            assert bool((got[wr] >= -1000.0).all()) and bool(torch.isfinite(got[wr]).all())
            _measured("la_emissions_from_logits", f"B={B},T={T},V={V},{'ctc' if variant else 'plain'},{tag},max_labels={max_labels}",
                      got[wr], ref[wr], e32[wr])
            assert torch.equal(got[wr] == -1000.0, ref[wr] == -1000.0), "the clamp applies at other entries than in float64"
            if tag == "neg_inf" and hi > lo and int(n_lab[0]) >= 2:
                assert float(got[0, 0, 1]) == 0.0 and float(got[0, 0, 2]) == -1000.0
            for b in range(B):
                if int(n_lab[b]) >= 6:
                    assert torch.equal(got[b, :, 4], got[b, :, 5])                 # a repeated label
                if int(n_lab[b]) > max_labels:
                    assert bool((got[b, :, 3:5] == -1000.0).all())                 # class ids hi + 1 and V
