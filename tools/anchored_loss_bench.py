"""Cost of the alignment loss on the windowed lattice (la_anchored_alignment_loss, csrc/la_anchor_loss.hip) beside la_multitask_loss.

    python tools/anchored_loss_bench.py [--runs 30] [--out profiles/anchored_loss.txt]

Shapes: B = 2 and B = 16 clips x 1500 frames x 21128 classes (+ the silence logit) x 26 labels (four lines of 6 / 7 / 6 / 7 characters, one
onset anchor per line within 1 s; logits 3 * randn).  Legs, alternated call by call in one process (caller-owned buffers, device events
around one call, a synchronise after each):
  * la_anchored_alignment_loss, loss only (no dlogits);
  * la_anchored_alignment_loss, loss + gradient;
  * la_multitask_loss(use_ce = 1, use_ctc = 1) with a gradient at the same shape: the existing entry, untouched by this feature.
Every number is the median of `runs` calls after a warm-up of 3; min .. max beside it.  The gradient kernel alone is timed by the library's
per-family timer in a second round of `runs` calls (mean), and placed against its one read + one write of the logits' rows.  The compiler's
resource lines of the new kernels come from the build's record (csrc/_obj/la_anchor_loss.hip.o.json).
"""
from __future__ import annotations

import ctypes
import json
import os

import torch

import benchlib as bl

HERE = os.path.dirname(os.path.abspath(__file__))
LINES = [6, 7, 6, 7]
T, V = 1500, 21128


def main(argv=None):
    args = bl.parse(bl.parser(), argv)
    report = bl.Report(args.out)
    say = report.say
    dev, Lb = bl.open_gpu()
    from lyricalignment_amd._lib import check, ptr, stream_ptr
    from lyricalignment_amd.utils.alignment import windows_from_anchors
    L = sum(LINES)
    say(f"# alignment loss on the windowed lattice on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a warm-up "
        f"of 3, legs alternated call by call, device events around one call, ms; {T} frames, {V} classes + silence logit, {L} labels")
    for B in (2, 16):
        g = torch.Generator().manual_seed(B)
        logits = (3.0 * torch.randn((B, T, V + 1), generator=g)).to(dev)
        labels = torch.randint(1, V, (B, L), generator=g, dtype=torch.int32)
        labels[:, 1] = labels[:, 0]
        labels[:, 9] = labels[:, 0]
        labels = labels.to(dev)
        n_labels = torch.full((B,), L, dtype=torch.int32, device=dev)
        starts = [sum(LINES[:i]) for i in range(len(LINES))]
        lo, hi = windows_from_anchors(L, T, onset_anchors=[(a, (T * (2 * a + 1) // (2 * L + 1)) * 0.02, 1.0) for a in starts])
        win_lo = torch.tensor([lo] * B, dtype=torch.int32).to(dev)
        win_hi = torch.tensor([hi] * B, dtype=torch.int32).to(dev)
        frame_labels = torch.full((B, T), -100, dtype=torch.int32)
        for n in range(L):
            frame_labels[:, T * (2 * n + 1) // (2 * L + 1): T * (2 * n + 2) // (2 * L + 1)] = labels[:, n: n + 1].cpu()
        frame_labels = frame_labels.to(dev)
        dlogits = torch.empty_like(logits)
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        nll = torch.empty((B,), dtype=torch.float64, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        losses3 = torch.empty((3,), dtype=torch.float32, device=dev)
        ws_a, need_a = bl.workspace(Lb, "la_anchored_alignment_loss_workspace_bytes", (B, T, L), dev)
        ws_m, need_m = bl.workspace(Lb, "la_multitask_loss_workspace_bytes", (B, T, L), dev)

        def anchored(with_grad):
            check(Lb.la_anchored_alignment_loss(ptr(logits), logits.stride(0), logits.stride(1), B, T, V, ptr(labels), L, ptr(n_labels), 0, L, 0, 0,
                                                0.0, ptr(win_lo), ptr(win_hi), win_lo.stride(0), 1.0, ptr(loss), ptr(nll), ptr(status),
                                                ptr(dlogits) if with_grad else 0, dlogits.stride(0), dlogits.stride(1), ptr(ws_a), need_a,
                                                stream_ptr()), "anchored_alignment_loss")

        def multitask():
            check(Lb.la_multitask_loss(ptr(logits), logits.stride(0), logits.stride(1), B, T, V, ptr(frame_labels), ptr(labels), L, ptr(n_labels),
                                       L, 1, 1, 1.0, ptr(losses3), ptr(dlogits), dlogits.stride(0), dlogits.stride(1), ptr(ws_m), need_m,
                                       stream_ptr()), "multitask_loss")

        legs = [("la_anchored_alignment_loss, loss only", lambda: anchored(False)),
                ("la_anchored_alignment_loss, loss + gradient", lambda: anchored(True)),
                ("la_multitask_loss(use_ce = 1, use_ctc = 1), loss + gradient", multitask)]
        bl.warm_up(legs)
        assert status.tolist() == [0] * B, status.tolist()
        times = bl.alternated(legs, args.runs, warmup=0)
        say(f"\n## B = {B}: loss {float(loss[0]):.4f}, workspace {need_a / 2 ** 20:.1f} MiB (la_multitask_loss: {need_m / 2 ** 20:.1f} MiB)")
        for name, t in times.items():
            say(bl.timed(name, bl.stat(t), 62))
        # the gradient kernel alone: the library's timer around its launch
        Lb.la_timer_reset(); Lb.la_timer_sample(1); Lb.la_timer_enable(b"anchored_loss_grad")
        for _ in range(args.runs):
            anchored(True)
        torch.cuda.synchronize()
        Lb.la_timer_disable()
        ms, count = ctypes.c_double(0), ctypes.c_int64(0)
        Lb.la_timer_read(ctypes.byref(ms), ctypes.byref(count))
        Lb.la_timer_reset()
        if count.value:
            per = ms.value / count.value
            moved = 2.0 * B * T * (V + 1) * 4
            say(f"gradient kernel alone (mean of {count.value}): {per:.3f} ms for one read + one write of {B * T} rows = {moved / 2 ** 30:.2f} GiB: "
                f"{moved / per / 1e9:.2f} TB/s")
        del logits, dlogits, ws_a, ws_m
    meta = os.path.join(HERE, "..", "lyricalignment_amd", "csrc", "_obj", "la_anchor_loss.hip.o.json")
    if os.path.exists(meta):
        say("\n## the compiler's resource lines of the new kernels (-Rpass-analysis=kernel-resource-usage)")
        keys = ("SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")
        with open(meta) as f:
            usage = json.load(f)["usage"]
        for name, u in usage.items():
            say(f"{name}: " + ", ".join(f"{k} {u.get(k)}" for k in keys if k in u))
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
