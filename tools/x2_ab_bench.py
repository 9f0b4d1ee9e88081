"""The f16x2 operand splits and product entries (csrc/la_f32x2.hip) beside another build of the library in one process: same bits, same
time.  The sibling of tools/gru_bench.py and tools/attn_ab_bench.py (the pairing is tools/ab_pair.py).

    python tools/x2_ab_bench.py --parent-lib <liblyricalign_hip.so of the parent commit> [--runs 40] [--control <copy of this build's library>]

Per leg both libraries run on the same inputs, each into its own outputs; every output is compared byte for byte before anything is timed;
then the two are alternated call by call, the one that goes first changing from pair to pair, device events around one call.  With --control
the same legs run once more against a copy of this build's own library: two loads of one code.  A leg passes when its outputs are bit-equal
and the excess of its median over the parent's median is no larger than the largest excess (either way round) the control shows on that leg.
Legs (the fine-tune shapes of tools/kbench.py x2): the plain split (with the operand maximum) and the transposed split (with column sums) of
24000 x 1024; la_gemm_f16x2 at 48000 x {3072, 4096, 1024} x 1024 with bias; la_gemm_f16x2_small at 1500 x 1024 x 1024 with its default slots
(split-K: the slot sum runs too); la_layernorm_f16x2 at 48000 x 1024.
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = ("la_split_f16x2_max", "la_split_f16x2_t_tmax", "la_gemm_f16x2", "la_gemm_f16x2_small", "la_layernorm_f16x2", "la_last_error")
# name, kind, M, N, K
LEGS = [("split 24000x1024", "split", 24000, 0, 1024), ("split_t 24000x1024", "split_t", 24000, 0, 1024),
        ("gemm_f16x2 48000x3072x1024", "gemm", 48000, 3072, 1024), ("gemm_f16x2 48000x4096x1024", "gemm", 48000, 4096, 1024),
        ("gemm_f16x2 48000x1024x1024", "gemm", 48000, 1024, 1024), ("gemm_f16x2_small 1500x1024x1024", "small", 1500, 1024, 1024),
        ("layernorm_f16x2 48000x1024", "ln", 48000, 0, 1024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=40)
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--control", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, ".."))
    import torch
    from lyricalignment_amd import _lib, f32x2
    from lyricalignment_amd._lib import lib, ptr, stream_ptr
    from ab_pair import load_sibling, measure_leg, verdict
    _lib.require_gpu()
    dev = torch.device("cuda:0")

    def make_call(L_, kind, M, N, K, x):
        """-> (call, outputs by name) for library L_ on the inputs x"""
        f16 = lambda *shape: torch.full(shape, -7.0, dtype=torch.float16, device=dev)
        f32 = lambda *shape: torch.full(shape, -7.0, dtype=torch.float32, device=dev)
        if kind == "split":
            outs = {"planes": f16(M, 2, K), "inv": f32(M), "max": torch.zeros(f32x2.OperandMax.WORDS, dtype=torch.int32, device=dev)}
            run = lambda: L_.la_split_f16x2_max(ptr(x["a"]), K, M, K, ptr(outs["planes"]), K, ptr(outs["inv"]), 0, ptr(outs["max"]), stream_ptr())
        elif kind == "split_t":
            mp = (M + 127) // 128 * 128
            outs = {"planes": f16(K, 2, mp), "inv": f32(K), "colsum": f32(K)}
            run = lambda: L_.la_split_f16x2_t_tmax(ptr(x["a"]), K, M, K, ptr(outs["planes"]), mp, ptr(outs["inv"]), 0, ptr(outs["colsum"]), None,
                                                   stream_ptr())
        elif kind == "ln":
            outs = {"planes": f16(M, 2, K), "inv": f32(M)}
            run = lambda: L_.la_layernorm_f16x2(ptr(x["a"]), K, M, K, ptr(x["g"]), ptr(x["b"]), ptr(outs["planes"]), K, ptr(outs["inv"]), stream_ptr())
        else:
            outs = {"c": f32(M, N)}
            fn, slots = (L_.la_gemm_f16x2, 1) if kind == "gemm" else (L_.la_gemm_f16x2_small, 0)
            run = lambda: fn(M, N, K, slots, ptr(x["ap"].planes), ptr(x["ap"].inv_scale), ptr(x["wp"].planes), ptr(x["wp"].inv_scale), ptr(outs["c"]), N,
                             ptr(x["bias"]), None, 0, _lib.EPI_BIAS, stream_ptr())

        def call():
            assert run() == 0, L_.la_last_error()
        return call, outs

    def ab(other, who):
        """-> {leg: (bit-equal, this median, other median)}"""
        res = {}
        for name, kind, M, N, K in LEGS:
            g = torch.Generator(device=dev).manual_seed(11 + M + N)
            x = {"a": torch.randn(M, K, device=dev, generator=g)}
            if kind == "ln":
                x.update(g=1 + 0.1 * torch.randn(K, device=dev, generator=g), b=0.1 * torch.randn(K, device=dev, generator=g))
            if kind in ("gemm", "small"):          # operands split by this build (the split legs compare the splits themselves)
                w = torch.randn(N, K, device=dev, generator=g) * K ** -0.5
                x.update(ap=f32x2.split(x["a"], K), wp=f32x2.split(w, K), bias=torch.randn(N, device=dev, generator=g) * 0.1)
            legs = [make_call(L_, kind, M, N, K, x) for L_ in (lib(), other)]
            res[name] = measure_leg(name, legs, args.runs, who)
            del legs, x
            torch.cuda.empty_cache()
        return res

    print(f"# f16x2 splits and products on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a warm-up of 3, the two "
          f"libraries alternated call by call (first place alternating), device events around one call", flush=True)
    got, ctl = ab(load_sibling(args.parent_lib, ENTRIES), "the parent's"), None
    if args.control:
        print("# the same against a copy of this build's own library", flush=True)
        ctl = ab(load_sibling(args.control, ENTRIES), "the copy's")
    return verdict(got, ctl)


if __name__ == "__main__":
    sys.exit(main())
