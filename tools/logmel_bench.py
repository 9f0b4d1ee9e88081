"""Cost of the 128-bin log-mel (whisper large-v3 / large-v3-turbo) beside the 80-bin one; csrc/la_logmel.hip.

    python tools/logmel_bench.py [--runs 30] [--parent-lib <liblyricalign_hip.so of the parent commit>] [--out profiles/logmel_128.txt]

32 clips x 480,000 samples (30 s), the flagship batch, synthetic waveforms.  Legs, alternated call by call (caller-owned buffers, cached
constants, device events around one call, a synchronise after each -- the protocol of tools/wide_lattice_bench.py):
  * la_logmel_f32_prepared: the 80-bin entry, the yardstick;
  * la_logmel_f32_prepared_n at n_mels = 80: the same launches through the entry that takes the bin count;
  * la_logmel_f32_prepared_n at n_mels = 128.
With --parent-lib the parent commit's la_logmel_f32_prepared runs in the same alternation (its output checked bit for bit against this
build's 80-bin legs), and both 80-bin legs are reported against the parent's min .. max.
Every number is the median of `runs` calls after a warm-up of 3; min .. max is printed next to it.  What the code predicts for 128 bins:
3,016 instead of 2,860 MFMAs per wave of a 64-frame tile (+5.5 %), 1.6 x the bytes written and 1.6 x the in-place floor pass.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
B, N = 32, 480000


def _time_once(torch, fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


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
    import numpy as np
    import torch
    from lyricalignment_amd import _lib
    from lyricalignment_amd._lib import SYMBOLS, lib, ptr, stream_ptr
    from lyricalignment_amd.audio_frontend import _device_constants, _device_tables
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    L = lib()
    rs = np.random.RandomState(0)
    t = np.arange(N) / 16000.0
    wave = np.stack([(rs.randn(N) * 0.05 + 0.3 * np.sin(2 * np.pi * (180 + 10 * b) * t)).astype(np.float32) * (0.1 + 0.03 * b) for b in range(B)])
    audio = torch.from_numpy(wave).to(dev)
    frames = N // 160

    def leg(L_, n_mels, by_count, consts):
        """-> (call, output); every leg owns its output and its workspace"""
        mel = torch.zeros((B, n_mels, frames), dtype=torch.float32, device=dev)
        need = ctypes.c_size_t(0)
        if by_count:
            assert L_.la_logmel_workspace_bytes_n(n_mels, B, N, ctypes.byref(need)) == 0
            entry, head = L_.la_logmel_f32_prepared_n, (n_mels,)
        else:
            assert L_.la_logmel_workspace_bytes(B, N, ctypes.byref(need)) == 0
            entry, head = L_.la_logmel_f32_prepared, ()
        ws = torch.empty((need.value,), dtype=torch.uint8, device=dev)

        def fn():
            assert entry(*head, ptr(audio), B, N, ptr(consts), ptr(mel), mel.stride(0), mel.stride(1), ptr(ws), need.value, stream_ptr()) == 0, \
                _lib.last_error()
        return fn, mel

    c80, c128 = _device_constants(0, 80), _device_constants(0, 128)
    legs = [("la_logmel_f32_prepared (80 bins)", leg(L, 80, False, c80)),
            ("la_logmel_f32_prepared_n, n_mels = 80", leg(L, 80, True, c80)),
            ("la_logmel_f32_prepared_n, n_mels = 128", leg(L, 128, True, c128))]
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("la_logmel_workspace_bytes", "la_logmel_f32_prepared", "la_logmel_constants_bytes", "la_logmel_constants"):
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = SYMBOLS[name]
        filt, win = _device_tables(0, 80)
        need = ctypes.c_size_t(0)
        assert parent.la_logmel_constants_bytes(ctypes.byref(need)) == 0
        cp = torch.empty((need.value,), dtype=torch.uint8, device=dev)
        assert parent.la_logmel_constants(ptr(filt), ptr(win), ptr(cp), need.value, stream_ptr()) == 0
        torch.cuda.synchronize()
        assert torch.equal(cp, c80), "the parent commit's constants differ from this build's 80-bin constants"
        legs.append(("parent commit: la_logmel_f32_prepared (80 bins)", leg(parent, 80, False, cp)))
    for _ in range(3):
        for _, (fn, _) in legs:
            fn()
    torch.cuda.synchronize()
    assert torch.equal(legs[0][1][1], legs[1][1][1]), "the two 80-bin entries differ"
    if args.parent_lib:
        assert torch.equal(legs[0][1][1], legs[3][1][1]), "80-bin output differs from the parent commit's"
    assert bool(torch.isfinite(legs[2][1][1]).all())
    ts = [[] for _ in legs]
    for _ in range(args.runs):
        for i, (_, (fn, _)) in enumerate(legs):
            ts[i].append(_time_once(torch, fn))
    say(f"# log-mel of {B} clips x {N} samples on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a warm-up of 3, "
        f"legs alternated call by call, device events around one call, ms")
    stats = {}
    base = statistics.median(ts[0])
    for (name, _), t_ in zip(legs, ts):
        m, lo, hi = statistics.median(t_), min(t_), max(t_)
        stats[name] = (m, lo, hi)
        say(f"{name:52s} {m:8.3f} ({lo:.3f} .. {hi:.3f})   {m / base:5.2f} x la_logmel_f32_prepared")
    say("the two 80-bin entries give the same bits" + ("; so does the parent commit's" if args.parent_lib else ""))
    moved = lambda n_mels: B * (N * 4 + 3 * n_mels * frames * 4) / 1e6        # waveform in, log-mel out, the floor pass in and out
    say(f"bytes moved per call: {moved(80):.0f} MB at 80 bins, {moved(128):.0f} MB at 128; MFMAs per wave of a tile 2860 and 3016")
    if args.parent_lib:
        pm, plo, phi = stats[legs[3][0]]
        for name, _ in legs[:2]:
            m = stats[name][0]
            where = "inside" if plo <= m <= phi else ("BELOW" if m < plo else "ABOVE")
            say(f"{name}: {m:.3f} against the parent's {pm:.3f} ({plo:.3f} .. {phi:.3f}): {where} its min .. max "
                f"({100 * (m / pm - 1):+.1f} % of its median)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
