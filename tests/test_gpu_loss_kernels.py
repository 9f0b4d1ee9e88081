"""la_multitask_loss (csrc/la_loss.hip: row statistics, the CTC alpha / beta lattice in its five instantiations, the dense gradient)
against the float64 restatement of tests/loss_reference.py, through the C ABI, on the case table that file shares with
tests/test_host_loss_kernels.py: every lattice kernel at both ends of its label range, one and two frames, the one-wave kernel's prefetch
blocks at their boundaries, a clip with exactly as many frames as it needs and one with a frame too few beside a feasible one, an empty
clip, a short clip in a wide launch, label classes that repeat side by side and at a distance or lie outside the vocabulary, V at the
256-column strides of the row kernels, logits with a common offset of +-1e4, a blank far above the row, rows of equal values, saturated
silence logits, and frame labels that are all -100 or outside 1..V-1.  Every case runs CE only, CTC only, both with scale 0.125 and
losses only (dlogits NULL), on dense rows and on pitched ones (row_stride V + 1 + 5, d_row_stride V + 1 + 9).

dlogits, losses and the workspace sit inside sentinel-filled allocations (the workspace exactly the queried size, 256-byte aligned): every
sentinel must survive, the pitch columns of dlogits included; the pitch columns of the logits hold 3e38 and must not be read.

Bounds.  Error against the float64 restatement must be <= 8 x E32 (FACTOR of test_gpu_row_kernels.py), E32 being the error of the same
quantity with the row normalisers taken by torch in float32 on the CPU (loss_reference.e32).  Losses: relative to max(|ref|, 1); dlogits:
relative to the tensor's largest |ref|.  One derived term: the one-wave lattice (S <= 64) takes the correction of log_add3 in float32,
which its comment (csrc/la_lattice.h) bounds at 1e-7 absolute per step, so a clip's nll may carry T * 1e-7 more -- losses[2] the mean over
the batch of T * 1e-7 / L_b -- and its occupancies, exp(alpha + beta + nll - lp) with alpha and beta summing to T steps, a relative
2 * T * 1e-7, that is 2 * T * 1e-7 * w on the gradient, w = scale / (B * L_b).  No other term.  Exact: +inf and NaN results, zero CTC rows
of infeasible and empty clips (with CE on: the rows of the CE-only call, bit for bit), column V with CE off, and for B = 1 the losses of
a losses-only call against those of the gradient call.  The gradient is never compared bit for bit between calls that run the lattice:
classes that repeat are summed with float atomics.

Every comparison prints `kernel case err E32 ratio`; the lines of one MI355X run are kept in profiles/loss_kernel_errors.txt.
"""
import ctypes
import math

import pytest
import torch

import loss_reference as LR
from test_gpu_row_kernels import FACTOR, NULL, Guard, _L, _ok, _same_bits, _st

pytestmark = pytest.mark.gpu

KERNEL = "la_multitask_loss"
PITCHES = ((0, 0), (5, 9))             # columns beyond V + 1 in a row of the logits / of dlogits
PAD = 3e38                             # what the pitch columns of the logits hold
LOG_ADD3 = 1e-7                        # the one-wave kernel's float32 correction per step (csrc/la_lattice.h, log_add3)


class Workspace:
    """Exactly `nbytes` at a 256-byte boundary with 256 sentinel bytes on both sides."""

    def __init__(self, nbytes):
        self.n = nbytes
        self.buf = torch.full((256 + nbytes + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + 256

    def check(self):
        torch.cuda.synchronize()
        host = self.buf.cpu()
        assert bool((host[:256] == 0x5A).all()) and bool((host[256 + self.n:] == 0x5A).all()), "a workspace guard byte was overwritten"


def _call(c, mode, pitch, grad=True, scale=None):
    """One call under MODES[mode] -> (losses [3], dlogits [B, T, V+1] or None) on the host, after every guard was checked."""
    L = _L()
    use_ce, use_ctc, mode_scale = LR.MODES[mode]
    scale = mode_scale if scale is None else scale
    B, T, V, Lmax = c["B"], c["T"], c["V"], c["max_labels"]
    ld, ldd = V + 1 + pitch[0], V + 1 + pitch[1]
    xp = torch.full((B, T, ld), PAD)
    xp[..., : V + 1] = c["x"]
    xd, fl, lab, nl = xp.cuda(), c["fl"].contiguous().cuda(), c["lab"].contiguous().cuda(), c["n_labels"].cuda()
    need = ctypes.c_size_t(0)
    _ok(L.la_multitask_loss_workspace_bytes(B, T, Lmax, ctypes.byref(need)), "multitask_loss_workspace_bytes")
    ws, losses = Workspace(need.value), Guard((3,))
    d = Guard((B, T, V + 1), (T * ldd, ldd, 1)) if grad else None
    _ok(L.la_multitask_loss(xd.data_ptr(), T * ld, ld, B, T, V, fl.data_ptr() if use_ce else NULL, lab.data_ptr() if use_ctc else NULL,
                            lab.stride(0), nl.data_ptr() if use_ctc else NULL, Lmax, use_ce, use_ctc, scale, losses.ptr,
                            d.ptr if grad else NULL, T * ldd if grad else 0, ldd if grad else 0, ws.ptr, need.value, _st()), KERNEL)
    ws.check()
    losses.check()
    if grad:
        d.check()
    return losses.get(), (d.get() if grad else None)


def _bounded(case, err, e32, extra=0.0):
    """err <= 8 E32 (+ the derived term); prints the figures first."""
    ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else math.inf)
    print(f"{KERNEL} {case} {err:.3e} {e32:.3e} {ratio:.2f}" + (f" (+{extra:.1e})" if extra else ""))
    assert err <= FACTOR * e32 + extra, (case, err, e32, extra)


def _check_losses(c, tag, mode, got, ref, y32):
    use_ce, use_ctc, _ = LR.MODES[mode]
    if use_ce:
        if math.isnan(float(ref[0])):
            assert math.isnan(float(got[0])), tag                                    # no frame with a label
        else:
            _bounded(f"{tag},ce", LR.rel_err(got[0:1], ref[0:1]), LR.rel_err(y32[0:1], ref[0:1]))
        _bounded(f"{tag},bce", LR.rel_err(got[1:2], ref[1:2]), LR.rel_err(y32[1:2], ref[1:2]))
    if use_ctc:
        if math.isinf(float(ref[2])):
            assert float(got[2]) == math.inf, tag                                    # a clip without a path
        else:
            extra = 0.0
            if 2 * c["max_labels"] + 1 <= 64:
                extra = sum(c["T"] * LOG_ADD3 / len(lab) for lab in c["labels"] if lab) / c["B"] / max(abs(float(ref[2])), 1.0)
            _bounded(f"{tag},ctc", LR.rel_err(got[2:3], ref[2:3]), LR.rel_err(y32[2:3], ref[2:3]), extra)


def _check_grad(c, tag, mode, got, ref, y32):
    use_ce, use_ctc, scale = LR.MODES[mode]
    V = c["V"]
    assert bool(torch.isfinite(got).all()), tag
    if not use_ce:
        assert not got[..., V].any(), tag                                             # the silence column belongs to the frame terms
    if use_ctc and not use_ce:
        for b in range(c["B"]):
            if LR.clip_state(c, b) != "ok":
                assert not got[b].any() and not ref[b].any(), (tag, b)                # exact zeros: no path, or no label
    if not ref.any():
        assert not got.any(), tag
        return
    extra = 0.0
    if use_ctc and 2 * c["max_labels"] + 1 <= 64:
        w = max((scale / (c["B"] * len(lab)) for b, lab in enumerate(c["labels"]) if LR.clip_state(c, b) == "ok"), default=0.0)
        extra = 2 * c["T"] * LOG_ADD3 * w / float(ref.abs().max())
    _bounded(f"{tag},dlogits", LR.grad_err(got, ref), LR.grad_err(y32, ref), extra)


@pytest.mark.parametrize("name", LR.CASE_NAMES)
def test_losses_and_gradient_match_the_float64_restatement(name):
    c = LR.make(name)
    odd_clips = [b for b in range(c["B"]) if LR.clip_state(c, b) != "ok"]
    for pitch in PITCHES:
        for mode in ("ce", "ctc", "both"):
            (ref_l, _, ref_d), (l32, _, d32) = LR.reference(name, mode)
            tag = f"{name},{mode},pitch={pitch[0]}+{pitch[1]}"
            got_l, got_d = _call(c, mode, pitch)
            _check_losses(c, tag, mode, got_l, ref_l, l32)
            _check_grad(c, tag, mode, got_d, ref_d, d32)
            only_l, _ = _call(c, mode, pitch, grad=False)                             # dlogits == NULL
            if c["B"] == 1:
                requested = [i for i in range(3) if not math.isnan(float(ref_l[i]))]
                _same_bits(only_l[requested], got_l[requested])
            _check_losses(c, tag + ",losses_only", mode, only_l, ref_l, l32)
            if mode == "both" and odd_clips:
                # a clip without a path or without labels takes no CTC gradient: with CE on, its rows are the CE-only call's, bit for bit
                _, ce_d = _call(c, "ce", pitch, scale=LR.MODES["both"][2])
                for b in odd_clips:
                    _same_bits(got_d[b], ce_d[b])
