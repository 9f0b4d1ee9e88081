"""Plain-torch restatement of the persistent GRU recurrence (csrc/la_gru.hip), evaluated in the dtype it is handed (float64: the
reference; float32 on the CPU: the yardstick), one step at a time.

Forward, DRIVEN: every kernel form writes every h_t to `out`, which is (or mirrors, bit for bit) the buffer the workgroups exchange h
through, so the recurrent product of step t is formed from the kernel's own row of the step before, read back from `out` and upcast
exactly -- a rounding flip of an exchanged h is then an input of the next step, not an error of it.  Per direction (forward t = 0..T-1,
reverse t = T-1..0) and clip:
    prod = W_hh h_exch          r = sigmoid(gi_r + prod_r + b_hr)     z = sigmoid(gi_z + prod_z + b_hz)
    hn = prod_n + b_hn          n = tanh(gi_n + r hn)                 carry_t = (1 - z) n + z carry_{t-1}
    ragged: carry_t = 0 at t >= n_frames[b], by a select             mish_t = mish(carry_t)   (torch's softplus threshold 20)
16-bit forms (gru_kernel<bf16 / f16>, gru_granule_kernel): the kernels keep hprev UNROUNDED in registers and round only the exchanged
copy, so the carry is the restatement's own unrounded value.  Float32 forms (gru_kernel<float>, gru_train_x2_kernel): h_exch and the
carry coincide (carry_from_exch=True: ordinary teacher forcing).  exch=None runs free: the restatement feeds itself, its exchanged copy
rounded to `round_to` if given.

Backward (la_gru_layer_bwd) is linear in dout once gates and out are given:
    dh = dout_t + dgh_{t+-1} W_hh + carry     dn = dh (1 - z)(1 - n^2)     dz = dh (h_prev - n) z (1 - z)     dr = dn hn r (1 - r)
    carry = dh z                              dgi = (dr, dz, dn)           dgh = (dr, dz, dn r)
"""
import math

import torch

OUTPUTS = ("h", "mish", "r", "z", "n", "hn")
TYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def driven_forward(gi, w_hh, b_hh, exch=None, n_frames=None, dtype=torch.float64, carry_from_exch=False, round_to=None):
    """gi [B][T][2][3H], w_hh [2][3H][H], b_hh [2][3H], exch [B][T][2H] (the kernel's `out`) or None -> {h, mish, r, z, n, hn}, each
    [B][T][2][H] in `dtype`."""
    B, T, _, H3 = gi.shape
    H = H3 // 3
    gi, W, b = gi.to(dtype), w_hh.to(dtype), b_hh.to(dtype)
    res = {k: torch.zeros(B, T, 2, H, dtype=dtype) for k in OUTPUTS}
    ex = None if exch is None else exch.to(dtype).reshape(B, T, 2, H)
    nf = None if n_frames is None else n_frames.to(torch.int64).reshape(B, 1)
    zero = torch.zeros(B, H, dtype=dtype)
    for d in range(2):
        carry, own, prev = zero, zero, None
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            hx = zero if prev is None else (own if ex is None else ex[:, prev, d])
            if nf is not None and prev is not None:
                hx = torch.where(prev < nf, hx, zero)           # rows past a clip's end are unspecified in `out`: h there is 0
            if carry_from_exch and prev is not None and ex is not None:
                carry = hx
            prod = hx @ W[d].T
            g = gi[:, t, d]
            r = torch.sigmoid(g[:, :H] + prod[:, :H] + b[d, :H])
            z = torch.sigmoid(g[:, H:2 * H] + prod[:, H:2 * H] + b[d, H:2 * H])
            hn = prod[:, 2 * H:] + b[d, 2 * H:]
            n = torch.tanh(g[:, 2 * H:] + r * hn)
            h = (1 - z) * n + z * carry
            if nf is not None:
                h = torch.where(t < nf, h, zero)
            carry = h
            own = h if round_to is None else h.to(round_to).to(dtype)
            for k, v in (("h", h), ("mish", torch.nn.functional.mish(h)), ("r", r), ("z", z), ("n", n), ("hn", hn)):
                res[k][:, t, d] = v
            prev = t
    return res


def backward(gates, out, dout, w_hh, dtype=torch.float64):
    """gates [B][T][2][4H] (r, z, n, hn), out / dout [B][T][2H], w_hh [2][3H][H] -> dgi, dgh [B][T][2][3H] in `dtype`."""
    B, T, _, H4 = gates.shape
    H = H4 // 4
    gt, W = gates.to(dtype), w_hh.to(dtype)
    o, do = out.to(dtype).reshape(B, T, 2, H), dout.to(dtype).reshape(B, T, 2, H)
    dgi, dgh = torch.zeros(B, T, 2, 3 * H, dtype=dtype), torch.zeros(B, T, 2, 3 * H, dtype=dtype)
    for d in range(2):
        carry, last = torch.zeros(B, H, dtype=dtype), None
        for t in (range(T - 1, -1, -1) if d == 0 else range(T)):            # the reverse of the forward scan
            tprev = t - 1 if d == 0 else t + 1                               # the forward pass's previous step
            r, z, n, hn = (gt[:, t, d, i * H:(i + 1) * H] for i in range(4))
            hp = o[:, tprev, d] if 0 <= tprev < T else torch.zeros(B, H, dtype=dtype)
            dh = do[:, t, d] + carry
            if last is not None:
                dh = dh + dgh[:, last, d] @ W[d]
            dn = dh * (1 - z) * (1 - n * n)
            dz = dh * (hp - n) * z * (1 - z)
            dr = dn * hn * r * (1 - r)
            carry = dh * z
            dgi[:, t, d] = torch.cat([dr, dz, dn], 1)
            dgh[:, t, d] = torch.cat([dr, dz, dn * r], 1)
            last = t
    return dgi, dgh


def torch_gru(gi, w_hh, b_hh, dtype=torch.float64):
    """torch.nn.GRU (bidirectional, batch_first) fed `gi` itself: input size 6H, W_ih = the two identity blocks, b_ih = 0.
    -> (out [B][T][2H], x): x is the leaf the module read (its gradient is dgi), the module hangs on out's graph."""
    B, T, _, H3 = gi.shape
    H = H3 // 3
    gru = torch.nn.GRU(2 * H3, H, num_layers=1, batch_first=True, bidirectional=True).to(dtype)
    with torch.no_grad():
        eye = torch.eye(H3, dtype=dtype)
        gru.weight_ih_l0.copy_(torch.cat([eye, torch.zeros_like(eye)], 1))
        gru.weight_ih_l0_reverse.copy_(torch.cat([torch.zeros_like(eye), eye], 1))
        gru.bias_ih_l0.zero_(); gru.bias_ih_l0_reverse.zero_()
        gru.weight_hh_l0.copy_(w_hh[0].to(dtype)); gru.weight_hh_l0_reverse.copy_(w_hh[1].to(dtype))
        gru.bias_hh_l0.copy_(b_hh[0].to(dtype)); gru.bias_hh_l0_reverse.copy_(b_hh[1].to(dtype))
    x = gi.to(dtype).reshape(B, T, 2 * H3).clone().requires_grad_(True)
    out, _ = gru(x)
    return out, x, gru


def ulp_T(ref, dt):
    """Spacing of the 16-bit type `dt` ('bf16' / 'f16') at |ref| (float64 tensor), subnormal range included."""
    mant, emin = {"bf16": (7, -126), "f16": (10, -14)}[dt]
    _, e = torch.frexp(ref.double().abs())                                   # |ref| = m 2^e, m in [0.5, 1)
    e = torch.where(ref == 0, torch.full_like(e, emin), e - 1).clamp(min=emin)
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e - mant)


def e32_step(ref64, ref32, mask=None):
    """Largest |float32 restatement - float64 restatement| per output, over the elements of `mask` ([B][T] or broadcastable)."""
    out = {}
    for k in ref64:
        d = (ref32[k].double() - ref64[k]).abs()
        if mask is not None:
            d = d[mask.expand(d.shape[:2])]
        d = d[~torch.isnan(d)]
        out[k] = float(d.max()) if d.numel() else 0.0
    return out


def rel_max(got, ref):
    """max |got - ref| / max(max |ref|, tiny): the error relative to the array's largest magnitude."""
    return float((got.double() - ref.double()).abs().max()) / max(float(ref.double().abs().max()), 1e-300)


# ---- cases --------------------------------------------------------------------------------------------------------------------------

FWD_CASES = ("gauss", "trained", "sat", "zero_rowcol", "wide_cols", "all_sat")
FWD_DEGENERATE = {"all_sat": ("h", "mish", "z", "hn")}     # gi_z = +1e4 everywhere: z = 1, h = 0 and hn = b_hn exactly in every arithmetic
BWD_CASES = ("gauss", "trained", "zero_rowcol", "wide_cols", "clip_scales", "dout_zero")
BWD_DEGENERATE = ("dout_zero",)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _round(w, wdt):
    return w.to(TYPES[wdt]).float()


def _weights(kind, H, wdt, g):
    w = torch.randn(2, 3 * H, H, generator=g) * (1.0 if kind == "trained" else H ** -0.5)
    if kind == "zero_rowcol":
        w[:, 5::H, :] = 0                             # unit 5's row of every gate
        w[:, :, 7] = 0                                # every gate's weight on h[7]
    if kind == "wide_cols":
        w = w * torch.exp2(torch.linspace(-20.0, 3.0, H)).reshape(1, 1, H)
    return _round(w, wdt)


def forward_case(kind, B, T, H, wdt="f32"):
    """(gi [B][T][2][3H], w_hh [2][3H][H] with values of the type wdt, b_hh [2][3H]), all float32.  gi and b_hh of one shape are one
    draw; the kinds change them as stated."""
    assert kind in FWD_CASES and H >= 64
    g = _gen(B, T, H)
    gi = torch.randn(B, T, 2, 3 * H, generator=g)
    b = torch.randn(2, 3 * H, generator=g) * 0.1
    w = _weights(kind, H, wdt, _gen(B, T, H, 1 + FWD_CASES.index(kind)))
    if kind == "all_sat":
        gi[..., H:2 * H] = 1e4
    if kind == "sat":
        # blocks of 4 units inside the first 64: gate (0 r, 1 z, 2 n) x value; the +1e4 block of z holds only at the inner steps, so
        # that a non-zero carry passes through it unchanged
        blocks = [(0, 30.0), (0, -30.0), (1, 30.0), (1, -30.0), (2, 30.0), (2, -30.0), (0, 1e4), (0, -1e4), (1, -1e4), (2, 1e4), (2, -1e4),
                  (0, math.inf), (0, -math.inf), (1, -math.inf), (2, math.inf), (2, -math.inf)]
        for i, (gate, v) in enumerate(blocks):
            gi[..., gate * H + 4 * i: gate * H + 4 * i + 4] = v
        inner = slice(2, max(2, T - 2))
        gi[:, inner, :, H + 32: H + 36] = 1e4          # units 32..35 (the -1e4 block of z at the outer steps)
    return gi, w, b


def ragged_lengths(B, T):
    """{T, 1, 2, T - 1, ...} over the clips."""
    pool = [T, 1, min(2, T), max(1, T - 1), max(1, T // 2), max(1, T - 2)]
    return torch.tensor([pool[i % len(pool)] for i in range(B)], dtype=torch.int32)


def with_nan_past_the_end(gi, n_frames):
    gi = gi.clone()
    for b, n in enumerate(n_frames.tolist()):
        gi[b, n:] = math.nan
    return gi


def foreign_clips(x, watched, salt=0):
    """A copy of x [B][...] in which every clip but `watched` holds NaN and +-1e30 in alternation."""
    y = x.clone()
    junk = torch.tensor([math.nan, 1e30, -1e30])
    for bb in range(x.shape[0]):
        if bb != watched:
            idx = (torch.arange(y[bb].numel()) + bb + salt) % 3
            y[bb] = junk[idx].reshape(y[bb].shape)
    return y


def backward_case(kind, B, T, H):
    """(gates, out, dout, w_hh) in float32: gates / out are the float64 free-running restatement on a Gaussian gi cast to float32 -- never
    a forward kernel's output."""
    assert kind in BWD_CASES
    g = _gen(B, T, H, 99)
    gi = torch.randn(B, T, 2, 3 * H, generator=g)
    b = torch.randn(2, 3 * H, generator=g) * 0.1
    dout = torch.randn(B, T, 2 * H, generator=g)
    w = _weights(kind, H, "f32", _gen(B, T, H, 50 + BWD_CASES.index(kind)))
    f = driven_forward(gi, w, b)
    gates = torch.cat([f["r"], f["z"], f["n"], f["hn"]], -1).float()
    out = f["h"].reshape(B, T, 2 * H).float()
    if kind == "clip_scales":
        dout[0] = 0
        dout[B - 1] *= 1e6
    if kind == "dout_zero":
        dout.zero_()
    return gates, out, dout, w


# ---- the documented layout of the workspace (csrc/la_gru.hip, la_gru_workspace_bytes) ----------------------------------------------

def workspace_layout(B, T, H):
    """[16-byte header: abort flag][counters [groups][2][T] u32], padded to 256 bytes, then the granule ring: the larger of the forward
    ring [groups][2][2 slots][16][H] x 8 bytes and -- where H is a multiple of 64 -- the backward ring [groups][2][2][(H/64)^2][16][64] x 8."""
    groups = (B + 15) // 16
    ctr = (16 + groups * 2 * T * 4 + 255) // 256 * 256
    fwd = groups * 2 * 2 * 16 * H * 8
    bwd = groups * 2 * 2 * (H // 64) ** 2 * 16 * 64 * 8 if H % 64 == 0 else 0
    return {"groups": groups, "counters": (16, groups * 2 * T), "ring": ctr, "fwd_ring": fwd, "bwd_ring": bwd, "total": ctr + max(fwd, bwd)}
