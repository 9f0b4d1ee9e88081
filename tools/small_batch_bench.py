"""float32 inference at 1-8 clips with option x2_small off and on (include/lyricalign.h; la_gemm_f16x2_small).

    python tools/small_batch_bench.py [--batches 1,2,4,8] [--rounds 3] [--iters 5] [--no-kernels] [--out FILE]

Whisper-medium with random-init weights (whisper_compat.build_model("medium")), float32, distinct synthetic 30 s clips.  One process; the
option alternates round by round (the order flips every round), every number is the median of device-event times around `iters` calls
with a synchronise after each.  Prints
  * model.align and whisper_model.embed_audio at each B: ms per call and per clip, encoder (embed_audio) / head (align - embed_audio) split;
  * per-shape kernel times of the float32 kernel (gemm_f32) and of la_gemm_f16x2_small (default split-K slots, the reduction included) at
    M = 1500 x B: QKV, out-proj, MLP-up, MLP-down, GRU input projection.
--batches 1 --rounds 1 --no-kernels --options 1 is the form to run under rocprofv3 --kernel-trace --stats.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SHAPES = [("qkv", 3072, 1024), ("out_proj", 1024, 1024), ("mlp_up", 4096, 1024), ("mlp_down", 1024, 4096), ("gru_in", 2304, 1024)]


def _time(fn, iters):
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def _wave(n, seed):
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    f = 180.0 + 40.0 * seed
    return (rs.randn(n) * 0.05 + 0.3 * np.sin(2 * np.pi * f * t) + 0.2 * np.sin(2 * np.pi * 2500 * t * (1 + 0.1 * t))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--options", default="0,1", help="x2_small values to run (1 alone: the form for a kernel trace of the new route)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from lyricalignment_amd import _lib, f32x2, ops, whisper_compat as wc
    from lyricalignment_amd.module.align_model import AlignModel
    _lib.require_gpu()
    torch.cuda.set_device(0)
    batches = [int(b) for b in args.batches.split(",")]
    opts = [int(o) for o in args.options.split(",")]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    wm = wc.build_model("medium", seed=3)
    model = AlignModel(wm, embed_dim=1024, hidden_dim=384, output_dim=21129, device="cuda:0", compute_dtype=torch.float32).eval()
    nb = max(batches)
    audios = [_wave(480000, s) for s in range(nb)]
    labels = torch.from_numpy(np.random.RandomState(1).randint(2, 403, size=(nb, 26)))
    mel = model._mel_of(audios).cuda()
    say(f"# float32 Whisper-medium, {torch.cuda.get_device_name(0)}; option x2_small 0 / 1 alternated over {args.rounds} rounds, "
        f"median of {args.iters} calls per round")
    res = {}
    with torch.no_grad():
        for B in batches:                                  # warm-up: engine packing, workspaces, first launches
            for opt in opts:
                with _lib.option("x2_small", opt):
                    model.align(audios[:B], labels[:B])
                    model.whisper_model.embed_audio(mel[:B])
        for r in range(args.rounds):
            for opt in (opts if r % 2 == 0 else opts[::-1]):
                with _lib.option("x2_small", opt):
                    for B in batches:
                        a = _time(lambda: model.align(audios[:B], labels[:B]), args.iters)
                        e = _time(lambda: model.whisper_model.embed_audio(mel[:B]), args.iters)
                        res.setdefault((B, opt), []).append((a, e))
    say("")
    say(f"{'B':>2} {'x2_small':>8} {'align ms':>9} {'/clip':>7} {'encoder':>8} {'head':>7}   align / encoder speed-up (0 -> 1)")
    for B in batches:
        med = {}
        for opt in opts:
            a = statistics.median(x[0] for x in res[(B, opt)])
            e = statistics.median(x[1] for x in res[(B, opt)])
            med[opt] = (a, e)
            extra = f"   {med[0][0] / a:.2f}x / {med[0][1] / e:.2f}x" if opt == 1 and 0 in med else ""
            say(f"{B:>2} {opt:>8} {a:>9.2f} {a / B:>7.2f} {e:>8.2f} {a - e:>7.2f}{extra}")
    if not args.no_kernels:
        say("")
        say(f"{'shape':>9} {'M':>6} {'N':>5} {'K':>5} {'slots':>5} {'gemm_f32 us':>12} {'f16x2_small us':>15} {'speed-up':>8}")
        for B in batches:
            M = 1500 * B
            for name, N, K in SHAPES:
                a = torch.randn(M, K, device="cuda")
                w = torch.randn(N, K, device="cuda") * K ** -0.5
                bias = torch.randn(N, device="cuda")
                A, W = f32x2.split(a, K), f32x2.split(w, K)
                out = torch.empty((M, N), device="cuda")
                t32, t16 = [], []
                for r in range(args.rounds):
                    for which in (("f32", "x2") if r % 2 == 0 else ("x2", "f32")):
                        if which == "f32":
                            t32.append(_time(lambda: ops.gemm(a, w, out, bias=bias), args.iters * 4))
                        else:
                            t16.append(_time(lambda: f32x2.gemm_small(A, W, out=out, bias=bias), args.iters * 4))
                m32, m16 = statistics.median(t32) * 1e3, statistics.median(t16) * 1e3
                say(f"{name:>9} {M:>6} {N:>5} {K:>5} {f32x2.slots_small(M, N, K):>5} {m32:>12.1f} {m16:>15.1f} {m32 / m16:>7.2f}x")
                del a, w, A, W, out
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
