"""Cost of the confidences on the lattice with optional lyric lines (la_alignment_posteriors_spans) beside la_alignment_posteriors; both are
instantiations of one kernel in csrc/la_posterior.hip, without and with the span code.

    python tools/span_confidence_bench.py [--runs 30] [--parent-tree DIR] [--ab-rounds 3] [--out profiles/span_confidence.txt]

On the same synthetic emissions at 32 clips x 1500 frames x 26 labels and at 1 x 5389 x 171 (caller-owned buffers, device events around one
call, a synchronise after each, the three calls alternated call by call):
  * la_alignment_posteriors                              -- the instantiation without any span code: the baseline;
  * la_alignment_posteriors_spans with no spans          -- every skip_from entry -1: what a span-free clip pays for the span instantiation;
  * la_alignment_posteriors_spans with four optional lines -- the first 26 labels as lines of 6 / 7 / 6 / 7 characters, each optional; the
    emissions plant every label except those of line 3.
Every number is the median of `runs` calls after a warm-up; min .. max is printed next to it.  The no-span outputs are checked bit for bit
against la_alignment_posteriors' before anything is timed.
--parent-tree DIR: a built checkout of the parent commit.  la_alignment_posteriors alone is then timed from both trees in fresh child
processes, alternated (this tree, parent, this tree, ...; `ab-rounds` processes each), BEFORE this process opens the GPU; the table gives
each process's median, the spread between the parent's own processes and whether the difference of the medians lies inside it.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(32, 1500, 26), (1, 5389, 171)]
LINES = [6, 7, 6, 7]
ABSENT_LINE = 2


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


def _inputs(torch, dev, B, T, L):
    """Emissions -rand * 12 - 1 with a 0.8 * 12 bonus on an even segmentation of the sung labels (all but line 3 of the four lines)."""
    g = torch.Generator().manual_seed(B + T + L)
    em = -torch.rand((B, T, L + 1), generator=g) * 12 - 1
    start = sum(LINES[:ABSENT_LINE])
    sung = [n for n in range(L) if not start <= n < start + LINES[ABSENT_LINE]]
    seg = T // (2 * len(sung) + 1)
    for i, n in enumerate(sung):
        em[:, (2 * i + 1) * seg:(2 * i + 2) * seg, 1 + n] += 9.6
    for i in range(len(sung) + 1):
        em[:, 2 * i * seg:(2 * i + 1) * seg, 0] += 9.6
    labels = torch.arange(1, L + 1, dtype=torch.int32).repeat(B, 1)
    n_labels = torch.full((B,), L, dtype=torch.int32)
    n_frames = torch.full((B,), T, dtype=torch.int32)
    return em.to(dev), labels.to(dev), n_labels.to(dev), n_frames.to(dev)


class _Plain:
    """la_alignment_posteriors on caller-owned buffers; onset / offset from la_viterbi_batch, once."""

    def __init__(self, torch, dev, B, T, L):
        from lyricalignment_amd._lib import check, lib, ptr, stream_ptr
        self.em, self.labels, self.n_labels, self.n_frames = _inputs(torch, dev, B, T, L)
        self.B, self.T, self.L = B, T, L
        self.on, self.off = (torch.empty((B, L), dtype=torch.int32, device=dev) for _ in range(2))
        self.score = torch.empty((B,), dtype=torch.float64, device=dev)
        self.vstatus = torch.empty((B,), dtype=torch.int32, device=dev)
        need = ctypes.c_size_t(0)
        check(lib().la_viterbi_workspace_bytes(B, T, L, ctypes.byref(need)))
        ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev)
        check(lib().la_viterbi_batch(ptr(self.em), self.em.stride(0), self.em.stride(1), ptr(self.labels), L, ptr(self.n_labels),
                                     ptr(self.n_frames), B, T, L, ptr(self.on), ptr(self.off), L, ptr(self.score), ptr(self.vstatus), ptr(ws),
                                     need.value, stream_ptr()), "viterbi_batch")
        torch.cuda.synchronize()
        self.need = ctypes.c_size_t(0)
        check(lib().la_alignment_posteriors_workspace_bytes(B, T, L, ctypes.byref(self.need)))
        self.ws = torch.empty((max(self.need.value, 16),), dtype=torch.uint8, device=dev)
        self.out = self.outputs(torch, dev)

    def outputs(self, torch, dev):
        B, L = self.B, self.L
        return [torch.empty((B, L), dtype=torch.float32, device=dev) for _ in range(3)] + [
            torch.empty((B,), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)]

    def __call__(self):
        from lyricalignment_amd._lib import check, lib, ptr, stream_ptr
        occ, onp, offp, log_z, status = self.out
        B, T, L = self.B, self.T, self.L
        check(lib().la_alignment_posteriors(ptr(self.em), self.em.stride(0), self.em.stride(1), ptr(self.labels), L, ptr(self.n_labels),
                                            ptr(self.n_frames), B, T, L, ptr(self.on), ptr(self.off), L, 2, ptr(occ), ptr(onp), ptr(offp),
                                            ptr(log_z), ptr(status), 0, 0, 0, ptr(self.ws), self.need.value, stream_ptr()), "alignment_posteriors")


def child(tree, runs):
    """la_alignment_posteriors from the package under `tree`: one JSON line {"B x T x L": [ms, ...]}."""
    sys.path.insert(0, tree)
    import torch
    from lyricalignment_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    out = {}
    for B, T, L in SHAPES:
        call = _Plain(torch, dev, B, T, L)
        for _ in range(3):
            call()
        out[f"{B} x {T} x {L}"] = [_time_once(torch, call) for _ in range(runs)]
    print("CHILD_JSON " + json.dumps(out), flush=True)


def ab_against_parent(parent_tree, rounds, runs, say):
    this_tree = os.path.abspath(os.path.join(HERE, ".."))
    res = {"this": [], "parent": []}
    for r in range(rounds):
        for which in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
            tree = this_tree if which == "this" else os.path.abspath(parent_tree)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--runs", str(runs)], capture_output=True, text=True,
                               timeout=300)
            line = next((l for l in p.stdout.splitlines() if l.startswith("CHILD_JSON ")), None)
            if p.returncode != 0 or line is None:
                raise RuntimeError(f"child for {tree} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            res[which].append(json.loads(line[len("CHILD_JSON "):]))
            print(f"[ab] round {r} {which} done", flush=True)
    say(f"## la_alignment_posteriors: this tree against the parent commit, fresh processes alternated, median of {runs} calls each (ms)")
    for key in res["this"][0]:
        mt = [statistics.median(c[key]) for c in res["this"]]
        mp = [statistics.median(c[key]) for c in res["parent"]]
        say(f"{key:>16}  this   " + " ".join(f"{v:8.3f}" for v in mt) + f"   median {statistics.median(mt):8.3f}")
        say(f"{key:>16}  parent " + " ".join(f"{v:8.3f}" for v in mp) + f"   median {statistics.median(mp):8.3f}   "
            f"spread between the parent's processes {max(mp) - min(mp):.3f} ({100 * (max(mp) - min(mp)) / statistics.median(mp):.2f} %)")
        d = statistics.median(mt) - statistics.median(mp)
        say(f"{'':>16}  difference this - parent {d:+.3f} ms ({100 * d / statistics.median(mp):+.2f} %): "
            + ("inside the parent's spread: equal" if abs(d) <= max(mp) - min(mp) else
               "outside the parent's spread, FASTER" if d < 0 else "OUTSIDE the parent's spread, SLOWER: a regression"))
    say("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.runs)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if args.parent_tree:
        ab_against_parent(args.parent_tree, args.ab_rounds, args.runs, say)       # children first: this process has not opened the GPU yet

    sys.path.insert(0, os.path.join(HERE, ".."))
    import torch
    from lyricalignment_amd import _lib
    from lyricalignment_amd._lib import check, lib, ptr, stream_ptr
    from lyricalignment_amd.utils.alignment import spans_from_lines
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    say(f"# confidences with optional lines on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after warm-up, "
        "device events, ms; boundary_window 2, no gamma output, skip_penalty 0")
    for B, T, L in SHAPES:
        plain = _Plain(torch, dev, B, T, L)
        skip_none = torch.full((B, L + 1), -1, dtype=torch.int32, device=dev)
        row = spans_from_lines(LINES, [True] * len(LINES)) + [-1] * (L - sum(LINES))
        skip_all = torch.tensor(row, dtype=torch.int32).repeat(B, 1).to(dev)
        # the span DP's frames for the span lattice (once, untimed)
        on_s, off_s = (torch.empty((B, L), dtype=torch.int32, device=dev) for _ in range(2))
        score_s, vstatus_s = torch.empty((B,), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
        need_v = ctypes.c_size_t(0)
        check(lib().la_viterbi_spans_workspace_bytes(B, T, L, ctypes.byref(need_v)))
        ws_v = torch.empty((max(need_v.value, 16),), dtype=torch.uint8, device=dev)
        check(lib().la_viterbi_spans_batch(ptr(plain.em), plain.em.stride(0), plain.em.stride(1), ptr(plain.labels), L, ptr(plain.n_labels),
                                           ptr(plain.n_frames), B, T, L, ptr(on_s), ptr(off_s), L, ptr(score_s), ptr(vstatus_s), ptr(skip_all),
                                           L + 1, 0.0, ptr(ws_v), need_v.value, stream_ptr()), "viterbi_spans_batch")
        need = ctypes.c_size_t(0)
        check(lib().la_alignment_posteriors_spans_workspace_bytes(B, T, L, ctypes.byref(need)))
        ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev)

        def span_outputs():
            return plain.outputs(torch, dev) + [torch.empty((B, L), dtype=torch.float32, device=dev),
                                                torch.empty((B, L + 1), dtype=torch.float32, device=dev)]

        out_n, out_a = span_outputs(), span_outputs()

        def spans(skip, on, off, out):
            occ, onp, offp, log_z, status, pres, skp = out
            check(lib().la_alignment_posteriors_spans(ptr(plain.em), plain.em.stride(0), plain.em.stride(1), ptr(plain.labels), L,
                                                      ptr(plain.n_labels), ptr(plain.n_frames), B, T, L, ptr(on), ptr(off), L, 2, ptr(skip), L + 1,
                                                      0.0, ptr(occ), ptr(onp), ptr(offp), ptr(pres), ptr(skp), ptr(log_z), ptr(status), 0, 0, 0,
                                                      ptr(ws), need.value, stream_ptr()), "alignment_posteriors_spans")

        no_spans = lambda: spans(skip_none, plain.on, plain.off, out_n)
        four_lines = lambda: spans(skip_all, on_s, off_s, out_a)
        for _ in range(3):
            plain(); no_spans(); four_lines()
        torch.cuda.synchronize()
        assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(plain.out, out_n)), "no-span outputs differ"
        assert int(out_a[4].abs().sum()) == 0 and int(vstatus_s.abs().sum()) == 0
        ends = [n for n, a in enumerate(row) if a >= 0]
        left_out = sorted({int(n) for n in (on_s < 0).nonzero()[:, 1].tolist()})
        tp, tn, ta = [], [], []
        for _ in range(args.runs):                           # alternated call by call
            tp.append(_time_once(torch, plain))
            tn.append(_time_once(torch, no_spans))
            ta.append(_time_once(torch, four_lines))
        (mp, lp, hp), (mn, ln, hn), (ma, la, ha) = _stat(tp), _stat(tn), _stat(ta)
        say(f"## {B} clips x {T} frames x {L} labels (workspace {need.value / 1e6:.1f} MB)")
        say(f"la_alignment_posteriors (baseline)                       {mp:8.3f} ({lp:.3f} .. {hp:.3f})")
        say(f"la_alignment_posteriors_spans, no spans                  {mn:8.3f} ({ln:.3f} .. {hn:.3f})   {mn / mp:5.2f} x   "
            f"{1e3 * (mn - mp) / (2 * T):+.3f} us per step and sweep")
        say(f"la_alignment_posteriors_spans, lines of 6/7/6/7 optional {ma:8.3f} ({la:.3f} .. {ha:.3f})   {ma / mp:5.2f} x   "
            f"{1e3 * (ma - mp) / (2 * T):+.3f} us per step and sweep")
        say(f"baseline's own spread (max - min) {hp - lp:.3f} ms; no-span outputs equal la_alignment_posteriors' bit for bit; labels the span DP "
            f"left out: {left_out}; span_skip_prob of clip 0 at the line ends {[round(float(out_a[6][0, n]), 4) for n in ends]}")
        say("")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
