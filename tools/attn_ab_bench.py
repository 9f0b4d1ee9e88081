"""The register-resident attention kernels (csrc/la_attention.hip, csrc/la_attention_f16x2.hip) beside another build of the library in one
process: same bits, same time.  The sibling of tools/gru_bench.py.

    python tools/attn_ab_bench.py --parent-lib <liblyricalign_hip.so of the parent commit> [--runs 40] [--control <copy of this build's library>]

Per leg both libraries run on the same inputs, each into its own outputs; every output is compared byte for byte before anything is timed;
then the two are alternated call by call, the one that goes first changing from pair to pair, device events around one call.  With --control
the same legs run once more against a copy of this build's own library: two loads of one code.  A leg passes when its outputs are bit-equal
and the excess of its median over the parent's median is no larger than the largest excess (either way round) the control shows on that leg.
Legs: the three 16-bit forms (bf16, f16, bf16 with exp2-domain scores) at 32 clips x 16 heads x 1500 (8 waves) and x 448 (4 waves); the
float32 kernel with lse, the f16x2 forward and the f16x2 backward at 16 x 16 x 1500.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = ("la_attention", "la_attention_lse_f32", "la_attention_f16x2_workspace_bytes", "la_attention_lse_f16x2",
           "la_attention_bwd_f16x2_workspace_bytes", "la_attention_bwd_f16x2", "la_last_error")
# name, kind, element type, LA_Q_LOG2, clips, frames
LEGS = [(f"{dt}{' q_log2' if ql else ''} 32x16x{T}", "16", dt, ql, 32, T) for T in (1500, 448) for dt, ql in (("bf16", 0), ("f16", 0), ("bf16", 1))]
LEGS += [("f32 + lse 16x16x1500", "f32", "f32", 0, 16, 1500), ("f16x2 forward 16x16x1500", "x2f", "f32", 0, 16, 1500),
         ("f16x2 backward 16x16x1500", "x2b", "f32", 0, 16, 1500)]
H = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=40)
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--control", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, ".."))
    import torch
    from lyricalignment_amd import _lib
    from lyricalignment_amd._lib import lib, ptr, stream_ptr
    from ab_pair import load_sibling, measure_leg, verdict
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    DT = {"f32": (torch.float32, _lib.LA_F32), "bf16": (torch.bfloat16, _lib.LA_BF16), "f16": (torch.float16, _lib.LA_F16)}

    def make_call(L_, kind, dt, qlog2, B, T, x):
        """-> (call, outputs by name) for library L_ on the inputs x"""
        d = 64 * H
        dtype, code = DT[dt]
        fill = lambda *shape: torch.full(shape, -7.0, dtype=dtype, device=dev)
        q, k, v = x["qkv"][:, :d], x["qkv"][:, d:2 * d], x["qkv"][:, 2 * d:]
        need = ctypes.c_size_t(0)
        if kind == "16":
            outs = {"out": fill(B * T, d)}
            run = lambda: L_.la_attention(code | (_lib.LA_Q_LOG2 if qlog2 else 0), ptr(x["qkv"]), 3 * d, ptr(outs["out"]), d, B, T, H, stream_ptr())
        elif kind == "f32":
            outs = {"out": fill(B * T, d), "lse": fill(B, H, T)}
            run = lambda: L_.la_attention_lse_f32(ptr(q), 3 * d, ptr(k), ptr(v), 3 * d, ptr(outs["out"]), d, B, T, T, H, 0, ptr(outs["lse"]), stream_ptr())
        elif kind == "x2f":
            assert L_.la_attention_f16x2_workspace_bytes(B, T, T, H, ctypes.byref(need)) == 0
            ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
            outs = {"out": fill(B * T, d), "lse": fill(B, H, T)}
            run = lambda: L_.la_attention_lse_f16x2(ptr(q), 3 * d, ptr(k), ptr(v), 3 * d, ptr(outs["out"]), d, B, T, T, H, 0, ptr(outs["lse"]), ptr(ws),
                                                    need.value, stream_ptr())
        else:
            assert L_.la_attention_bwd_f16x2_workspace_bytes(B, T, T, H, ctypes.byref(need)) == 0
            ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
            outs = {"dqkv": fill(B * T, 3 * d)}
            g = outs["dqkv"]
            run = lambda: L_.la_attention_bwd_f16x2(ptr(q), 3 * d, ptr(k), ptr(v), 3 * d, ptr(x["o"]), d, ptr(x["do"]), d, ptr(g[:, :d]), 3 * d,
                                                    ptr(g[:, d:2 * d]), ptr(g[:, 2 * d:]), 3 * d, B, T, T, H, 0, ptr(x["lse"]), ptr(ws), need.value, stream_ptr())

        def call():
            assert run() == 0, L_.la_last_error()
        return call, outs

    def ab(other, who):
        """-> {leg: (bit-equal, this median, other median)}"""
        res = {}
        for name, kind, dt, qlog2, B, T in LEGS:
            d = 64 * H
            g = torch.Generator(device=dev).manual_seed(7 + T + B)
            qkv = torch.randn(B * T, 3 * d, device=dev, generator=g)
            qkv[:, :d] *= 0.35 if dt == "f32" else (0.125 * 1.4426950408889634 if qlog2 else 0.125)
            x = {"qkv": qkv.to(DT[dt][0])}
            if kind == "x2b":           # o and lse of this build's forward, a random upstream gradient
                fwd, fo = make_call(lib(), "x2f", dt, 0, B, T, x)
                fwd()
                x.update(o=fo["out"], lse=fo["lse"], do=torch.randn(B * T, d, device=dev, generator=g) * 1e-3)
            legs = [make_call(L_, kind, dt, qlog2, B, T, x) for L_ in (lib(), other)]
            res[name] = measure_leg(name, legs, args.runs, who)
            del legs, x
            torch.cuda.empty_cache()
        return res

    print(f"# attention kernels on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a warm-up of 3, the two libraries "
          f"alternated call by call (first place alternating), device events around one call", flush=True)
    got, ctl = ab(load_sibling(args.parent_lib, ENTRIES), "the parent's"), None
    if args.control:
        print("# the same against a copy of this build's own library", flush=True)
        ctl = ab(load_sibling(args.control, ENTRIES), "the copy's")
    return verdict(got, ctl)


if __name__ == "__main__":
    sys.exit(main())
