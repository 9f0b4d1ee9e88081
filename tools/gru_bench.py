"""Every form of the GRU recurrence kernels (csrc/la_gru.hip) beside the parent commit's library: same bits, same time.

    python tools/gru_bench.py [--runs 30] [--parent-lib <liblyricalign_hip.so of the parent commit>] [--out profiles/gru_refactor.txt]

One leg per kernel form at T = 1500, H = 384, selected the way the form table of tests/test_gpu_gru_kernels.py selects it (an option only
where the documented dispatch would pick another form):
    F7  gru_granule_kernel           la_gru_layer, bf16 and f16, B = 32 and 64; la_gru_layer_ragged, bf16, B = 32
    F6  gru_kernel<16-bit>, 8 waves  la_gru_layer, bf16, B = 16 and B = 1; B = 16 with gru_fence = 1 (the release / acquire form)
    F5  gru_kernel<16-bit>, 4 waves  la_gru_layer, bf16, B = 32, gru_nw = 4
    F1  gru_kernel<float>            la_gru_layer, f32, B = 2
    F2  gru_train_x2_kernel          la_gru_layer, f32, B = 32
    F3  gru_train_x2_kernel, gates   la_gru_layer_train_fwd, B = 8
    B1  gru_bwd_x2_kernel<6>         la_gru_layer_bwd, B = 8
    B2  gru_bwd_kernel               la_gru_layer_bwd, B = 2
With --parent-lib every leg runs this build and the parent commit's library in one process on the same inputs (each library owns its
outputs and its workspace): every output -- out, out_mish, gates, dgi, dgh -- is compared byte for byte before anything is timed, then the
two are alternated call by call, the one that goes first changing from pair to pair, with device events around one call.  Reported per leg: median (min .. max) of `runs` calls after a
warm-up of 3, and where the median lies against the parent's min .. max.  Rule: outputs bit-equal, median not above the parent's maximum.
Given a copy of this build's own library as --parent-lib, the same legs show what two loads of one code differ by.
--out: a file that already has a section "## 2." keeps its other sections; only that section's body is replaced.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
T, H = 1500, 384
# name, entry, dtype, batch, options, ragged
LEGS = [
    ("F7 bf16 B=32", "layer", "bf16", 32, {}, False),
    ("F7 bf16 B=64", "layer", "bf16", 64, {}, False),
    ("F7 f16 B=32", "layer", "f16", 32, {}, False),
    ("F7 f16 B=64", "layer", "f16", 64, {}, False),
    ("F7 ragged bf16 B=32", "layer", "bf16", 32, {}, True),
    ("F6 bf16 B=16", "layer", "bf16", 16, {}, False),
    ("F6 bf16 B=1", "layer", "bf16", 1, {}, False),
    ("F5 bf16 B=32, gru_nw=4", "layer", "bf16", 32, {"gru_nw": 4}, False),
    ("F1 f32 B=2", "layer", "f32", 2, {}, False),
    ("F2 f32 B=32", "layer", "f32", 32, {}, False),
    ("F3 train_fwd B=8", "train", "f32", 8, {}, False),
    ("B1 bwd B=8", "bwd", "f32", 8, {}, False),
    ("B2 bwd B=2", "bwd", "f32", 2, {}, False),
    ("F6 fence bf16 B=16, gru_fence=1", "layer", "bf16", 16, {"gru_fence": 1}, False),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    sys.path.insert(0, os.path.join(HERE, ".."))
    import torch
    from lyricalignment_amd import _lib
    from lyricalignment_amd._lib import lib, ptr, stream_ptr
    from ab_pair import alternate, load_sibling, same_bytes
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    libs = [("", lib())]
    if args.parent_lib:
        libs.append(("parent commit: ", load_sibling(args.parent_lib, ("la_gru_workspace_bytes", "la_gru_layer", "la_gru_layer_ragged",
                                                                        "la_gru_layer_train_fwd", "la_gru_layer_bwd", "la_set_option",
                                                                        "la_get_option", "la_last_error"))))
    DT = {"f32": (torch.float32, _lib.LA_F32), "bf16": (torch.bfloat16, _lib.LA_BF16), "f16": (torch.float16, _lib.LA_F16)}

    def pin(L_, opts):
        """options are per library: pinned on the one about to be called -> what they were"""
        prev = {}
        for k, v in opts.items():
            old = ctypes.c_int64(0)
            assert L_.la_get_option(k.encode(), ctypes.byref(old)) == 0
            prev[k] = int(old.value)
            assert L_.la_set_option(k.encode(), v) == 0
        return prev

    def make_call(L_, entry, dt, B, opts, inputs):
        """-> (call, outputs by name); the call checks its status, the time-out flag is the last output"""
        dtype, code = DT[dt]
        need = ctypes.c_size_t(0)
        assert L_.la_gru_workspace_bytes(B, T, H, ctypes.byref(need)) == 0
        ws = torch.empty((need.value,), dtype=torch.uint8, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        fill = lambda shape, d: torch.full(shape, -7.0, dtype=d, device=dev)
        if entry == "bwd":
            outs = {"dgi": fill((B, T, 2, 3 * H), torch.float32), "dgh": fill((B, T, 2, 3 * H), torch.float32)}
            gates, out, dout, w = inputs

            def run():
                return L_.la_gru_layer_bwd(ptr(gates), ptr(out), ptr(dout), ptr(w), ptr(outs["dgi"]), ptr(outs["dgh"]), B, T, H, ptr(ws), need.value,
                                           ptr(flag), stream_ptr())
        elif entry == "train":
            outs = {"out": fill((B, T, 2 * H), torch.float32), "gates": fill((B, T, 2, 4 * H), torch.float32)}
            gi, w, b, _ = inputs

            def run():
                return L_.la_gru_layer_train_fwd(ptr(gi), ptr(w), ptr(b), ptr(outs["out"]), ptr(outs["gates"]), B, T, H, ptr(ws), need.value, ptr(flag),
                                                 stream_ptr())
        else:
            outs = {"out": fill((B, T, 2 * H), dtype), "out_mish": fill((B, T, 2 * H), dtype)}
            gi, w, b, n_frames = inputs

            def run():
                if n_frames is not None:
                    return L_.la_gru_layer_ragged(code, ptr(gi), ptr(w), ptr(b), ptr(outs["out"]), ptr(outs["out_mish"]), B, T, ptr(n_frames), H, ptr(ws),
                                                  need.value, ptr(flag), stream_ptr())
                return L_.la_gru_layer(code, ptr(gi), ptr(w), ptr(b), ptr(outs["out"]), ptr(outs["out_mish"]), B, T, H, ptr(ws), need.value, ptr(flag),
                                       stream_ptr())

        def call(_held=(inputs, ws)):
            prev = pin(L_, opts)
            rc = run()
            pin(L_, prev)
            assert rc == 0, L_.la_last_error()
        outs["timeout_flag"] = flag
        return call, outs

    say(f"# GRU recurrence kernels on {torch.cuda.get_device_name(0)}, T = {T}, H = {H}: median (min .. max) of {args.runs} calls after a warm-up "
        f"of 3, the two libraries alternated call by call (first place alternating), device events around one call, ms")
    broken = []
    for name, entry, dt, B, opts, ragged in LEGS:
        g = torch.Generator(device=dev).manual_seed(1000 + B)
        rnd = lambda *shape: torch.randn(shape, generator=g, device=dev, dtype=torch.float32)
        w32 = rnd(2, 3 * H, H) / H ** 0.5
        if entry == "bwd":
            # the saved gates and h of a training forward (this build's; F3 compares them with the parent's), a random upstream gradient
            gi, b = rnd(B, T, 2, 3 * H), rnd(2, 3 * H) * 0.1
            fwd, fo = make_call(lib(), "train", "f32", B, {}, (gi, w32, b, None))
            fwd()
            torch.cuda.synchronize()
            assert int(fo["timeout_flag"]) == 0
            inputs = (fo["gates"], fo["out"], rnd(B, T, 2 * H), w32)
            del gi
        else:
            n_frames = None
            if ragged:
                n_frames = torch.randint(T // 3, T + 1, (B,), generator=torch.Generator().manual_seed(B), dtype=torch.int32)
                n_frames[0] = T
                n_frames = n_frames.to(dev)
            inputs = (rnd(B, T, 2, 3 * H), w32.to(DT[dt][0]), rnd(2, 3 * H) * 0.1, n_frames)
        legs = [(who + name,) + make_call(L_, entry, dt, B, opts, inputs) for who, L_ in libs]
        for _ in range(3):
            for _, fn, _ in legs:
                fn()
        torch.cuda.synchronize()
        for who, _, outs in legs:
            assert int(outs["timeout_flag"]) == 0, f"{who}: a bounded wait timed out"
        equal = None
        if len(legs) == 2:
            valid = None
            if ragged:                                # rows past a clip's length are unspecified
                valid = (torch.arange(T, device=dev)[None, :] < inputs[3][:, None])[:, :, None]
            differ = []
            for k in legs[0][2]:
                a, b_ = legs[0][2][k], legs[1][2][k]
                if valid is not None and a.dim() == 3:
                    a, b_ = torch.where(valid, a, torch.zeros_like(a)), torch.where(valid, b_, torch.zeros_like(b_))
                if not same_bytes(a, b_):
                    differ.append(k)
            equal = not differ
            if differ:
                broken.append(f"{name}: {', '.join(differ)} differ from the parent commit's")
        ts = alternate([fn for _, fn, _ in legs], args.runs)
        m, lo, hi = statistics.median(ts[0]), min(ts[0]), max(ts[0])
        line = f"{name:34s} {m:8.3f} ({lo:.3f} .. {hi:.3f})   {1e3 * m / T:6.3f} us per step"
        if len(legs) == 2:
            pm, plo, phi = statistics.median(ts[1]), min(ts[1]), max(ts[1])
            where = "inside" if plo <= m <= phi else ("BELOW" if m < plo else "ABOVE")
            line += (f"   against the parent's {pm:.3f} ({plo:.3f} .. {phi:.3f}): {where} its min .. max ({100 * (m / pm - 1):+.1f} % of its median); "
                     f"outputs {'bit-equal' if equal else 'DIFFER'}")
            if m > phi:
                broken.append(f"{name}: median {m:.3f} ms above the parent's maximum {phi:.3f} ms")
        say(line)
        del legs, inputs
        torch.cuda.empty_cache()
    if len(libs) == 2:
        say(f"verdict: {'every leg bit-equal and not above the parent maximum' if not broken else 'RULE BROKEN: ' + '; '.join(broken)}")
    if args.out:
        # a record that already has numbered sections keeps them: only the body of its section 2 (up to "## 3.") is replaced
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        old = open(args.out).read().split("\n") if os.path.exists(args.out) else []
        heads = [i for i, l in enumerate(old) if l.startswith("## 2.")]
        if heads:
            a = heads[0] + 1
            while a < len(old) and old[a].startswith("##"):
                a += 1
            b = next((i for i in range(a, len(old)) if old[i].startswith("## 3.")), len(old))
            lines = old[:a] + [""] + lines + [""] + old[b:]
        with open(args.out, "w") as f:
            f.write("\n".join(lines).rstrip("\n") + "\n")
    return 1 if broken else 0


if __name__ == "__main__":
    sys.exit(main())
