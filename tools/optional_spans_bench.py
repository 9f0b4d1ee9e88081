"""Cost of the alignment DP with optional lyric lines (la_viterbi_spans_batch) beside la_viterbi_batch; both are
instantiations of one kernel in csrc/la_viterbi.hip, without and with the span code.

    python tools/optional_spans_bench.py [--runs 30] [--out profiles/optional_spans.txt]

On the same synthetic emissions at 32 clips x 1500 frames x 26 labels (caller-owned buffers, device events around one call, a
synchronise after each, the three calls alternated call by call):
  * la_viterbi_batch                          -- the instantiation without any span code: the baseline;
  * la_viterbi_spans_batch with no spans      -- every skip_from entry -1: what a span-free clip pays for the span instantiation;
  * la_viterbi_spans_batch with every line optional -- the 26 labels as four lines of 6 / 7 / 6 / 7 characters, each optional; the emissions
    plant lines 1, 2 and 4, so the jump over line 3 is taken.
Every number is the median of `runs` calls after a warm-up; min .. max is printed next to it.  The no-span outputs are checked bit for
bit against la_viterbi_batch's before anything is timed.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
B, T, L = 32, 1500, 26
LINES = [6, 7, 6, 7]
PRESENT = [True, True, False, True]


def _time_once(torch, fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def _stat(ts):
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    sys.path.insert(0, os.path.join(HERE, ".."))
    import torch
    from lyricalignment_amd import _lib
    from lyricalignment_amd._lib import check, lib, ptr, stream_ptr
    from lyricalignment_amd.utils.alignment import spans_from_lines
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")

    # emissions -rand * 12 - 1 with a 0.8 * 12 bonus on an even segmentation of the SUNG labels (lines 1, 2 and 4)
    g = torch.Generator().manual_seed(B + T + L)
    em = -torch.rand((B, T, L + 1), generator=g) * 12 - 1
    sung, pos = [], 0
    for n_chars, here in zip(LINES, PRESENT):
        sung += list(range(pos, pos + n_chars)) if here else []
        pos += n_chars
    seg = T // (2 * len(sung) + 1)
    for i, n in enumerate(sung):
        em[:, (2 * i + 1) * seg:(2 * i + 2) * seg, 1 + n] += 9.6
    for i in range(len(sung) + 1):
        em[:, 2 * i * seg:(2 * i + 1) * seg, 0] += 9.6
    em = em.to(dev)
    labels = torch.arange(1, L + 1, dtype=torch.int32).repeat(B, 1).to(dev)
    n_labels = torch.full((B,), L, dtype=torch.int32, device=dev)
    n_frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    skip_none = torch.full((B, L + 1), -1, dtype=torch.int32, device=dev)
    skip_all = torch.tensor(spans_from_lines(LINES, [True] * len(LINES)), dtype=torch.int32).repeat(B, 1).to(dev)

    def outputs():
        return (torch.empty((B, L), dtype=torch.int32, device=dev), torch.empty((B, L), dtype=torch.int32, device=dev),
                torch.empty((B,), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))

    out_v, out_n, out_a = outputs(), outputs(), outputs()
    need_v, need_s = ctypes.c_size_t(0), ctypes.c_size_t(0)
    check(lib().la_viterbi_workspace_bytes(B, T, L, ctypes.byref(need_v)))
    check(lib().la_viterbi_spans_workspace_bytes(B, T, L, ctypes.byref(need_s)))
    ws_v = torch.empty((max(need_v.value, 16),), dtype=torch.uint8, device=dev)
    ws_s = torch.empty((max(need_s.value, 16),), dtype=torch.uint8, device=dev)

    def vit():
        on, off, score, status = out_v
        check(lib().la_viterbi_batch(ptr(em), em.stride(0), em.stride(1), ptr(labels), L, ptr(n_labels), ptr(n_frames), B, T, L, ptr(on),
                                     ptr(off), L, ptr(score), ptr(status), ptr(ws_v), need_v.value, stream_ptr()), "viterbi_batch")

    def spans(skip, out):
        on, off, score, status = out
        check(lib().la_viterbi_spans_batch(ptr(em), em.stride(0), em.stride(1), ptr(labels), L, ptr(n_labels), ptr(n_frames), B, T, L, ptr(on),
                                           ptr(off), L, ptr(score), ptr(status), ptr(skip), L + 1, 0.0, ptr(ws_s), need_s.value, stream_ptr()),
              "viterbi_spans_batch")

    for _ in range(3):
        vit(); spans(skip_none, out_n); spans(skip_all, out_a)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out_v, out_n)), "no-span outputs differ from la_viterbi_batch"
    assert int(out_a[3].abs().sum()) == 0
    left_out = sorted({int(n) for n in (out_a[0] < 0).nonzero()[:, 1].tolist()})
    tv, tn, ta = [], [], []
    for _ in range(args.runs):                           # alternated call by call
        tv.append(_time_once(torch, vit))
        tn.append(_time_once(torch, lambda: spans(skip_none, out_n)))
        ta.append(_time_once(torch, lambda: spans(skip_all, out_a)))
    (mv, lv, hv), (mn, ln, hn), (ma, la, ha) = _stat(tv), _stat(tn), _stat(ta)
    say(f"# alignment DP with optional lines on {torch.cuda.get_device_name(0)}; {B} clips x {T} frames x {L} labels, median (min .. max) of "
        f"{args.runs} calls after warm-up, device events, ms")
    say(f"la_viterbi_batch (baseline)                      {mv:8.3f} ({lv:.3f} .. {hv:.3f})")
    say(f"la_viterbi_spans_batch, no spans                 {mn:8.3f} ({ln:.3f} .. {hn:.3f})   {mn / mv:5.2f} x   {1e3 * (mn - mv) / T:+.3f} us per frame")
    say(f"la_viterbi_spans_batch, lines of 6/7/6/7 optional {ma:7.3f} ({la:.3f} .. {ha:.3f})   {ma / mv:5.2f} x   {1e3 * (ma - mv) / T:+.3f} us per frame")
    say(f"baseline's own spread (max - min) {hv - lv:.3f} ms; no-span outputs equal la_viterbi_batch's bit for bit; labels left out with the "
        f"spans: {left_out}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
