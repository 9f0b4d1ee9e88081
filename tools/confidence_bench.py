"""Cost of the alignment confidences (la_alignment_posteriors, csrc/la_posterior.hip) and proof that the default path is untouched.

    python tools/confidence_bench.py [--runs 20] [--parent-tree DIR] [--ab-rounds 3] [--out profiles/confidence.txt]

For (B, T, L) = (32, 1500, 26), (1, 1500, 26) and (1, 5389, 171), Whisper-medium with random-init weights:
  * la_alignment_posteriors alone and la_viterbi_batch alone on the same synthetic emissions (caller-owned buffers, device events around one
    call, a synchronise after each);
  * model.align with and without return_confidence, float32 and bfloat16, alternated call by call.
Every number is the median of `runs` calls after a warm-up of every shape; min .. max is printed next to it.
--parent-tree DIR: a built checkout of the parent commit.  model.align WITHOUT return_confidence is then timed from both trees in fresh
child processes, alternated (this tree, parent, this tree, ...; `ab-rounds` processes each), BEFORE this process opens the GPU; the table
gives each process's median and the spread between the parent's own processes.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(32, 1500, 26), (1, 1500, 26), (1, 5389, 171)]


def _wave(n, seed):
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    f = 180.0 + 40.0 * (seed % 8)
    return (rs.randn(n) * 0.05 + 0.3 * np.sin(2 * np.pi * f * t) + 0.2 * np.sin(2 * np.pi * 2500 * t * (1 + 0.1 * t))).astype(np.float32)


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


def _workload(B, T, L):
    """Distinct synthetic clips whose head sees T frames (2 mel frames per head frame, 160 samples per mel frame) and L labels each."""
    audios = [_wave(T * 2 * 160, s) for s in range(B)]
    labels = np.random.RandomState(1).randint(2, 403, size=(B, L))
    for b in range(B):
        for n in range(1, L):
            while labels[b, n] == labels[b, n - 1]:
                labels[b, n] = labels[b, n] % 400 + 2
    return audios, labels


def _models(dtypes):
    import torch
    from lyricalignment_amd import whisper_compat as wc
    from lyricalignment_amd.module.align_model import AlignModel
    wm = wc.build_model("medium", seed=3)
    return {name: AlignModel(wm, embed_dim=1024, hidden_dim=384, output_dim=21129, device="cuda:0",
                             compute_dtype=getattr(torch, name)).eval() for name in dtypes}


def child(tree, runs):
    """Plain model.align from the package under `tree`: one JSON line {"<dtype> B<B>": [ms, ...]}."""
    sys.path.insert(0, tree)
    import torch
    from lyricalignment_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    out = {}
    models = _models(["bfloat16", "float32"])
    with torch.no_grad():
        for name, B in (("bfloat16", 32), ("float32", 1)):
            audios, labels = _workload(B, 1500, 26)
            lab = torch.from_numpy(labels)
            for _ in range(3):
                models[name].align(audios, lab)
            out[f"{name} B{B}"] = [_time_once(torch, lambda: models[name].align(audios, lab)) for _ in range(runs)]
    print("CHILD_JSON " + json.dumps(out), flush=True)


def ab_against_parent(parent_tree, rounds, runs, say):
    this_tree = os.path.abspath(os.path.join(HERE, ".."))
    res = {"this": [], "parent": []}
    for r in range(rounds):
        for which in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
            tree = this_tree if which == "this" else os.path.abspath(parent_tree)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--runs", str(runs)], capture_output=True, text=True,
                               timeout=600)
            line = next((l for l in p.stdout.splitlines() if l.startswith("CHILD_JSON ")), None)
            if p.returncode != 0 or line is None:
                raise RuntimeError(f"child for {tree} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            res[which].append(json.loads(line[len("CHILD_JSON "):]))
            print(f"[ab] round {r} {which} done", flush=True)
    say(f"## model.align WITHOUT return_confidence: this tree against the parent commit, fresh processes alternated, median of {runs} calls each (ms)")
    for key in res["this"][0]:
        mt = [statistics.median(c[key]) for c in res["this"]]
        mp = [statistics.median(c[key]) for c in res["parent"]]
        say(f"{key:>14}  this   " + " ".join(f"{v:8.3f}" for v in mt) + f"   median {statistics.median(mt):8.3f}")
        say(f"{key:>14}  parent " + " ".join(f"{v:8.3f}" for v in mp) + f"   median {statistics.median(mp):8.3f}   "
            f"spread between the parent's processes {max(mp) - min(mp):.3f} ({100 * (max(mp) - min(mp)) / statistics.median(mp):.2f} %)")
        d = statistics.median(mt) - statistics.median(mp)
        say(f"{'':>14}  difference this - parent {d:+.3f} ms ({100 * d / statistics.median(mp):+.2f} %): "
            + ("inside the parent's spread: equal" if abs(d) <= max(mp) - min(mp) else "OUTSIDE the parent's spread"))
    say("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
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
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    say(f"# alignment confidences on {torch.cuda.get_device_name(0)}; median (min .. max) of {args.runs} calls after warm-up, device events, ms")
    say("")
    say("## kernels alone (synthetic emissions -rand * 12 - 1 with a 0.8 * 12 bonus on an even segmentation, caller-owned buffers)")
    say(f"{'B':>3} {'T':>5} {'L':>4} {'la_viterbi_batch':>28} {'la_alignment_posteriors':>30} {'us per step and sweep':>22} {'workspace MB':>13}")
    for B, T, L in SHAPES:
        g = torch.Generator().manual_seed(B + T + L)
        em = -torch.rand((B, T, L + 1), generator=g) * 12 - 1
        seg = T // (2 * L + 1)
        for n in range(L):
            em[:, (2 * n + 1) * seg:(2 * n + 2) * seg, 1 + n] += 9.6
        em = em.to(dev)
        labels = torch.arange(1, L + 1, dtype=torch.int32).repeat(B, 1).to(dev)
        n_labels = torch.full((B,), L, dtype=torch.int32, device=dev)
        n_frames = torch.full((B,), T, dtype=torch.int32, device=dev)
        on = torch.empty((B, L), dtype=torch.int32, device=dev)
        off = torch.empty_like(on)
        score = torch.empty((B,), dtype=torch.float64, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        occ = torch.empty((B, L), dtype=torch.float32, device=dev)
        onp, offp = torch.empty_like(occ), torch.empty_like(occ)
        log_z = torch.empty_like(score)
        pstatus = torch.empty_like(status)
        need_v, need_p = ctypes.c_size_t(0), ctypes.c_size_t(0)
        check(lib().la_viterbi_workspace_bytes(B, T, L, ctypes.byref(need_v)))
        check(lib().la_alignment_posteriors_workspace_bytes(B, T, L, ctypes.byref(need_p)))
        ws_v = torch.empty((max(need_v.value, 16),), dtype=torch.uint8, device=dev)
        ws_p = torch.empty((need_p.value,), dtype=torch.uint8, device=dev)

        def vit():
            check(lib().la_viterbi_batch(ptr(em), em.stride(0), em.stride(1), ptr(labels), L, ptr(n_labels), ptr(n_frames), B, T, L, ptr(on),
                                         ptr(off), L, ptr(score), ptr(status), ptr(ws_v), need_v.value, stream_ptr()), "viterbi_batch")

        def post():
            check(lib().la_alignment_posteriors(ptr(em), em.stride(0), em.stride(1), ptr(labels), L, ptr(n_labels), ptr(n_frames), B, T, L,
                                                ptr(on), ptr(off), L, 2, ptr(occ), ptr(onp), ptr(offp), ptr(log_z), ptr(pstatus), 0, 0, 0,
                                                ptr(ws_p), need_p.value, stream_ptr()), "alignment_posteriors")

        for _ in range(3):
            vit(); post()
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0 and int(pstatus.abs().sum()) == 0
        tv, tp = [], []
        for _ in range(args.runs):                       # alternated call by call
            tv.append(_time_once(torch, vit))
            tp.append(_time_once(torch, post))
        (mv, lv, hv), (mp, lp, hp) = _stat(tv), _stat(tp)
        say(f"{B:>3} {T:>5} {L:>4} {mv:>10.3f} ({lv:.3f} .. {hv:.3f}) {mp:>12.3f} ({lp:.3f} .. {hp:.3f}) {1e3 * mp / (2 * T):>22.3f} {need_p.value / 1e6:>13.1f}")
        say(f"{'':>14} occupancy of the run: {float(occ.min()):.3f} .. {float(occ.max()):.3f}")
    say("")
    say("## model.align, Whisper-medium (random-init weights), with and without return_confidence, alternated call by call")
    say(f"{'dtype':>9} {'B':>3} {'T':>5} {'L':>4} {'plain':>28} {'return_confidence':>30} {'added ms':>9} {'added %':>8}")
    models = _models(["bfloat16", "float32"])
    with torch.no_grad():
        for name, model in models.items():
            for B, T, L in SHAPES:
                audios, labels = _workload(B, T, L)
                lab = torch.from_numpy(labels)
                for _ in range(3):
                    model.align(audios, lab)
                    model.align(audios, lab, return_confidence=True)
                t0, t1 = [], []
                for _ in range(args.runs):
                    t0.append(_time_once(torch, lambda: model.align(audios, lab)))
                    t1.append(_time_once(torch, lambda: model.align(audios, lab, return_confidence=True)))
                (m0, l0, h0), (m1, l1, h1) = _stat(t0), _stat(t1)
                got_T = int(model.align(audios, lab, return_frames=True)[1].max())
                say(f"{name:>9} {B:>3} {T:>5} {L:>4} {m0:>10.2f} ({l0:.2f} .. {h0:.2f}) {m1:>12.2f} ({l1:.2f} .. {h1:.2f}) {m1 - m0:>9.2f} {100 * (m1 - m0) / m0:>7.2f}%"
                    f"   (last offset frame {got_T})")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
