"""The emission head and the row losses (csrc/la_head.hip, la_elementwise.hip, la_train_elem.hip, la_anchor_loss.hip, la_loss.hip -- the
users of csrc/la_row.h) beside another build of the library in one process: same bits, same time.  The sibling of tools/x2_ab_bench.py
(the pairing is tools/ab_pair.py).

    python tools/head_ab_bench.py --parent-lib <liblyricalign_hip.so of the parent commit> [--runs 30] [--control <copy of this build's library>]

Per leg both libraries run on the same inputs, each into its own outputs and workspace; every output is compared byte for byte before
anything is timed; then the two are alternated call by call, device events around one call.  With --control the same legs run once more
against a copy of this build's own library: two loads of one code.  A leg passes when its outputs are bit-equal and the excess of its
median over the parent's median is no larger than the largest excess (either way round) the control shows on that leg.
Legs: la_fc_emissions at 32 x 1500 rows, K = 768, V = 21129, 26 labels in bf16, f16 and float32; la_fc_emissions_x2 and bf16 with option
gemm_loop = 99 (the ping-pong loop) at the same shape; la_emissions_from_logits at 16 x 1500 x 21129, both variants; la_cross_entropy_f32
at 64 x 51865; la_anchored_alignment_loss and la_multitask_loss at B = 2 and 16, 1500 frames, 21128 classes, 26 labels (the shapes of
tools/anchored_loss_bench.py), with and without the gradient.  The gradient of la_multitask_loss with CTC on is summed with float atomics
and is not bit-stable between two runs of one library: that leg compares the losses, and reports the largest gradient difference.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = ("la_fc_emissions_workspace_bytes", "la_fc_emissions", "la_fc_emissions_x2_workspace_bytes", "la_fc_emissions_x2", "la_set_option",
           "la_emissions_from_logits", "la_cross_entropy_f32", "la_anchored_alignment_loss_workspace_bytes", "la_anchored_alignment_loss",
           "la_multitask_loss_workspace_bytes", "la_multitask_loss", "la_last_error")
LINES = [6, 7, 6, 7]
NL = sum(LINES)
T, V, K = 1500, 21128, 768


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--control", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, ".."))
    import torch
    from lyricalignment_amd import _lib, f32x2
    from lyricalignment_amd._lib import lib, ptr, stream_ptr
    from lyricalignment_amd.utils.alignment import windows_from_anchors
    from ab_pair import load_sibling, measure_leg, verdict
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    f32 = lambda *shape: torch.full(shape, -7.0, dtype=torch.float32, device=dev)

    def workspace(query, *a):
        need = ctypes.c_size_t(0)
        assert query(*a, ctypes.byref(need)) == 0
        return torch.empty((need.value,), dtype=torch.uint8, device=dev), need.value

    def labels_of(B, g, hi):
        lab = torch.randint(1, hi, (B, NL), generator=g, dtype=torch.int32)
        lab[:, 1] = lab[:, 0]
        lab[:, 9] = lab[:, 0]
        return lab.to(dev), torch.full((B,), NL, dtype=torch.int32, device=dev)

    def fc_inputs(dtype):
        B, g = 32, torch.Generator(device=dev).manual_seed(5)
        x = {"B": B, "act": torch.randn(B * T, K, device=dev, generator=g).to(dtype),
             "w": (torch.randn(V + 1, K, device=dev, generator=g) * (2.0 / K ** 0.5)).to(dtype), "bias": 0.5 * torch.randn(V + 1, device=dev, generator=g)}
        x["lab"], x["n"] = labels_of(B, torch.Generator().manual_seed(6), V)
        return x

    def fc_call(L_, x, kind):
        B, code = x["B"], _lib.dtype_code(x["act"].dtype)
        outs = {"em": f32(B, T, NL + 1)}
        tail = lambda ws, need: (B, T, K, V + 1, _lib.LA_VARIANT_CTC, ptr(x["lab"]), NL, ptr(x["n"]), NL, ptr(outs["em"]), T * (NL + 1), NL + 1, ptr(ws),
                                 need, stream_ptr())
        if kind == "x2":
            ws, need = workspace(L_.la_fc_emissions_x2_workspace_bytes, B, T, K, V + 1, NL)
            run = lambda: L_.la_fc_emissions_x2(ptr(x["act"]), K, ptr(x["w"]), ptr(x["bias"]), ptr(x["wp"].planes), ptr(x["wp"].inv_scale), *tail(ws, need))
        else:
            ws, need = workspace(L_.la_fc_emissions_workspace_bytes, code, B, T, K, V + 1, NL)
            run = lambda: L_.la_fc_emissions(code, ptr(x["act"]), K, ptr(x["w"]), ptr(x["bias"]), *tail(ws, need))
        return run, outs

    def from_logits_call(L_, x, variant):
        B = x["B"]
        outs = {"em": f32(B, T, NL + 1)}
        lg = x["logits"]
        run = lambda: L_.la_emissions_from_logits(ptr(lg), lg.stride(0), lg.stride(1), B, T, V + 1, variant, ptr(x["lab"]), NL, ptr(x["n"]), NL,
                                                  ptr(outs["em"]), T * (NL + 1), NL + 1, stream_ptr())
        return run, outs

    def ce_call(L_, x):
        lg, R, C = x["logits"], x["logits"].shape[0], x["logits"].shape[1]
        outs = {"loss2": f32(2), "row_ws": f32(2 * R), "dlogits": f32(R, C)}
        run = lambda: L_.la_cross_entropy_f32(ptr(lg), C, R, C, ptr(x["target"]), 1.0, ptr(outs["loss2"]), ptr(outs["row_ws"]), ptr(outs["dlogits"]), C,
                                              stream_ptr())
        return run, outs

    def loss_inputs(B):
        g = torch.Generator(device=dev).manual_seed(B)
        x = {"B": B, "logits": 3.0 * torch.randn((B, T, V + 1), device=dev, generator=g)}
        x["lab"], x["n"] = labels_of(B, torch.Generator().manual_seed(B + 100), V)
        starts = [sum(LINES[:i]) for i in range(len(LINES))]
        lo, hi = windows_from_anchors(NL, T, onset_anchors=[(a, (T * (2 * a + 1) // (2 * NL + 1)) * 0.02, 1.0) for a in starts])
        x["win_lo"], x["win_hi"] = (torch.tensor([w] * B, dtype=torch.int32).to(dev) for w in (lo, hi))
        fl = torch.full((B, T), -100, dtype=torch.int32)
        for n in range(NL):
            fl[:, T * (2 * n + 1) // (2 * NL + 1): T * (2 * n + 2) // (2 * NL + 1)] = x["lab"][:, n: n + 1].cpu()
        x["frame_labels"] = fl.to(dev)
        return x

    def anchored_call(L_, x, grad):
        B, lg = x["B"], x["logits"]
        outs = {"loss": f32(1), "nll": torch.zeros(B, dtype=torch.float64, device=dev), "status": torch.full((B,), -7, dtype=torch.int32, device=dev)}
        if grad:
            outs["dlogits"] = f32(*lg.shape)
        ws, need = workspace(L_.la_anchored_alignment_loss_workspace_bytes, B, T, NL)
        run = lambda: L_.la_anchored_alignment_loss(ptr(lg), lg.stride(0), lg.stride(1), B, T, V, ptr(x["lab"]), NL, ptr(x["n"]), 0, NL, 0, 0, 0.0,
                                                    ptr(x["win_lo"]), ptr(x["win_hi"]), x["win_lo"].stride(0), 1.0, ptr(outs["loss"]), ptr(outs["nll"]),
                                                    ptr(outs["status"]), ptr(outs.get("dlogits")), lg.stride(0), lg.stride(1), ptr(ws), need, stream_ptr())
        return run, outs

    def multitask_call(L_, x, ctc, grad, extra):
        """extra: receives the gradient where it is not part of the bit comparison (CTC on: float atomics)"""
        B, lg = x["B"], x["logits"]
        outs = {"losses": f32(3)}
        dl = f32(*lg.shape) if grad else None
        if grad:
            (extra if ctc else outs)["dlogits"] = dl
        ws, need = workspace(L_.la_multitask_loss_workspace_bytes, B, T, NL)
        run = lambda: L_.la_multitask_loss(ptr(lg), lg.stride(0), lg.stride(1), B, T, V, ptr(x["frame_labels"]), ptr(x["lab"]), NL, ptr(x["n"]), NL, 1,
                                           int(ctc), 1.0, ptr(outs["losses"]), ptr(dl), lg.stride(0), lg.stride(1), ptr(ws), need, stream_ptr())
        return run, outs

    def ab(other, who):
        """-> {leg: (bit-equal, this median, other median)}"""
        res, both = {}, (lib(), other)

        def leg(name, make):
            def checked(L_):
                run, outs = make(L_)

                def call():
                    assert run() == 0, L_.la_last_error()
                return call, outs
            res[name] = measure_leg(name, [checked(L_) for L_ in both], args.runs, who)
            torch.cuda.empty_cache()

        for tag, dtype in (("bf16", torch.bfloat16), ("f16", torch.float16), ("f32", torch.float32)):
            x = fc_inputs(dtype)
            leg(f"fc_emissions {tag}", lambda L_: fc_call(L_, x, "plain"))
            if tag == "f32":
                x["wp"] = f32x2.split(x["w"], K)                      # split by this build: the x2 A/B tool compares the splits themselves
                leg("fc_emissions_x2", lambda L_: fc_call(L_, x, "x2"))
            if tag == "bf16":
                for L_ in both:
                    assert L_.la_set_option(b"gemm_loop", 99) == 0
                leg("fc_emissions bf16 gemm_loop=99", lambda L_: fc_call(L_, x, "plain"))
                for L_ in both:
                    assert L_.la_set_option(b"gemm_loop", 0) == 0
            del x
        x = loss_inputs(16)
        for variant, tag in ((_lib.LA_VARIANT_CTC, "ctc"), (_lib.LA_VARIANT_PLAIN, "plain")):
            leg(f"emissions_from_logits {tag}", lambda L_: from_logits_call(L_, x, variant))
        del x
        g = torch.Generator(device=dev).manual_seed(64)
        x = {"logits": 3.0 * torch.randn((64, 51865), device=dev, generator=g), "target": torch.randint(0, 51865, (64,), device=dev, generator=g)}
        x["target"][5] = -100
        leg("cross_entropy 64x51865", lambda L_: ce_call(L_, x))
        del x
        for B in (2, 16):
            x = loss_inputs(B)
            for grad in (False, True):
                leg(f"anchored_loss B={B}{' +grad' if grad else ''}", lambda L_: anchored_call(L_, x, grad))
            for ctc, grad in ((False, False), (False, True), (True, False), (True, True)):
                extras = []
                name = f"multitask B={B} ce{'+ctc' if ctc else ''}{' +grad' if grad else ''}"

                def make(L_):
                    extras.append({})
                    return multitask_call(L_, x, ctc, grad, extras[-1])
                leg(name, make)
                if ctc and grad:
                    d = float((extras[0]["dlogits"] - extras[1]["dlogits"]).abs().max())
                    print(f"{name:32s} gradient (float atomics, outside the bit comparison): max |difference| against {who} {d:.3e}, "
                          f"max |gradient| {float(extras[0]['dlogits'].abs().max()):.3e}", flush=True)
            del x
        return res

    print(f"# emission head and row losses on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a warm-up of 3, the two "
          f"libraries alternated call by call (first place alternating), device events around one call", flush=True)
    got, ctl = ab(load_sibling(args.parent_lib, ENTRIES), "the parent's"), None
    if args.control:
        print("# the same against a copy of this build's own library", flush=True)
        ctl = ab(load_sibling(args.control, ENTRIES), "the copy's")
    return verdict(got, ctl)


if __name__ == "__main__":
    sys.exit(main())
