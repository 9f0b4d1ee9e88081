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

import numpy as np
import torch

import benchlib as bl

SHAPES = [(32, 1500, 26), (1, 1500, 26), (1, 5389, 171)]


def _wave(n, seed):
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    f = 180.0 + 40.0 * (seed % 8)
    return (rs.randn(n) * 0.05 + 0.3 * np.sin(2 * np.pi * f * t) + 0.2 * np.sin(2 * np.pi * 2500 * t * (1 + 0.1 * t))).astype(np.float32)


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
    from lyricalignment_amd import whisper_compat as wc
    from lyricalignment_amd.module.align_model import AlignModel
    wm = wc.build_model("medium", seed=3)
    return {name: AlignModel(wm, embed_dim=1024, hidden_dim=384, output_dim=21129, device="cuda:0",
                             compute_dtype=getattr(torch, name)).eval() for name in dtypes}


def child(tree, runs):
    """Plain model.align from the package under `tree`: one JSON line {"<dtype> B<B>": [ms, ...]}."""
    bl.open_gpu(tree)
    out = {}
    models = _models(["bfloat16", "float32"])
    with torch.no_grad():
        for name, B in (("bfloat16", 32), ("float32", 1)):
            audios, labels = _workload(B, 1500, 26)
            lab = torch.from_numpy(labels)
            out[f"{name} B{B}"] = bl.alternated([("", lambda: models[name].align(audios, lab))], runs)[""]
    bl.child_json(out)


def main(argv=None):
    ap = bl.parser()
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = bl.parse(ap, argv, runs=20)
    if args.child:
        return child(args.child, args.runs)
    report = bl.Report(args.out)
    say = report.say
    if args.parent_tree:                                     # children first: this process has not opened the GPU yet
        res = bl.ab_children(__file__, bl.ROOT, args.parent_tree, args.ab_rounds, args.runs, timeout=600)
        say(f"## model.align WITHOUT return_confidence: this tree against the parent commit, fresh processes alternated, median of {args.runs} calls each (ms)")
        for key in res["this"][0]:
            for line in bl.against_parent_processes(key, [p[key] for p in res["this"]], [p[key] for p in res["parent"]]):
                say(line)
        say("")

    dev, lib = bl.open_gpu()
    say(f"# alignment confidences on {torch.cuda.get_device_name(0)}; median (min .. max) of {args.runs} calls after warm-up, device events, ms")
    say("")
    say("## kernels alone (synthetic emissions -rand * 12 - 1 with a 0.8 * 12 bonus on an even segmentation, caller-owned buffers)")
    say(f"{'B':>3} {'T':>5} {'L':>4} {'la_viterbi_batch':>28} {'la_alignment_posteriors':>30} {'us per step and sweep':>22} {'workspace MB':>13}")
    for B, T, L in SHAPES:
        g = torch.Generator().manual_seed(B + T + L)
        em = -torch.rand((B, T, L + 1), generator=g) * 12 - 1              # the labels' bonus only: silence keeps its draw
        seg = T // (2 * L + 1)
        for n in range(L):
            em[:, (2 * n + 1) * seg:(2 * n + 2) * seg, 1 + n] += 9.6
        c = bl.case(em.to(dev), *bl.sheet(B, T, L, dev))
        vit = bl.dp_leg(lib, "viterbi", c)
        post = bl.posterior_leg(lib, "alignment_posteriors", c, (vit[1]["onset"], vit[1]["offset"]))
        legs = [("vit", vit), ("post", post)]
        bl.warm_up(legs)
        assert bl.ok(vit[1]) and bl.ok(post[1])
        ts = bl.alternated(legs, args.runs, warmup=0)
        (mv, lv, hv), (mp, lp, hp) = bl.stat(ts["vit"]), bl.stat(ts["post"])
        say(f"{B:>3} {T:>5} {L:>4} {mv:>10.3f} ({lv:.3f} .. {hv:.3f}) {mp:>12.3f} ({lp:.3f} .. {hp:.3f}) {1e3 * mp / (2 * T):>22.3f} "
            f"{post[0].workspace_bytes / 1e6:>13.1f}")
        occ = post[1]["occupancy"]
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
                ts = bl.alternated([("plain", lambda: model.align(audios, lab)), ("conf", lambda: model.align(audios, lab, return_confidence=True))],
                                   args.runs)
                (m0, l0, h0), (m1, l1, h1) = bl.stat(ts["plain"]), bl.stat(ts["conf"])
                got_T = int(model.align(audios, lab, return_frames=True)[1].max())
                say(f"{name:>9} {B:>3} {T:>5} {L:>4} {m0:>10.2f} ({l0:.2f} .. {h0:.2f}) {m1:>12.2f} ({l1:.2f} .. {h1:.2f}) {m1 - m0:>9.2f} {100 * (m1 - m0) / m0:>7.2f}%"
                    f"   (last offset frame {got_T})")
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
