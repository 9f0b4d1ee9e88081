"""Cost of the confidences on the lattice with optional lyric lines (la_alignment_posteriors_spans) beside la_alignment_posteriors; both are
instantiations of one kernel in csrc/la_posterior.hip, without and with the span code.

    python tools/span_confidence_bench.py [--runs 30] [--quick] [--parent-tree DIR] [--ab-rounds 3] [--out profiles/span_confidence.txt]

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

import torch

import benchlib as bl

LEGS = ("la_alignment_posteriors (baseline)", "la_alignment_posteriors_spans, no spans", "la_alignment_posteriors_spans, lines of {} optional")
SHAPES, LINES = [(32, 1500, 26), (1, 5389, 171)], [6, 7, 6, 7]
QUICK, QUICK_LINES = [bl.QUICK_ONE_WAVE[:3], bl.QUICK_MULTI_WAVE[:3]], [2, 2, 2, 2]
ABSENT_LINE = 2


def leg_table(quick=False):
    """Per shape, the names the report gives the legs."""
    lines = QUICK_LINES if quick else LINES
    return [[name.format("/".join(map(str, lines))) for name in LEGS] for _ in (QUICK if quick else SHAPES)]


def _plain(lib, dev, B, T, L, lines):
    """-> the shape's inputs (every label planted but those of line 3), la_viterbi_batch's (onset, offset), la_alignment_posteriors on them."""
    start = sum(lines[:ABSENT_LINE])
    sung = [n for n in range(L) if not start <= n < start + lines[ABSENT_LINE]]
    c = bl.case(bl.planted(B, T, L, sung, B + T + L, dev), *bl.sheet(B, T, L, dev))
    dp, out = bl.dp_leg(lib, "viterbi", c)
    bl.warm_up([("", dp)], 1)
    frames = (out["onset"], out["offset"])
    return c, frames, bl.posterior_leg(lib, "alignment_posteriors", c, frames)


def child(tree, runs):
    """la_alignment_posteriors from the package under `tree`: one JSON line {"B x T x L": [ms, ...]}."""
    dev, lib = bl.open_gpu(tree)
    out = {}
    for B, T, L in SHAPES:
        leg = _plain(lib, dev, B, T, L, LINES)[2]
        out[f"{B} x {T} x {L}"] = bl.alternated([("", leg)], runs)[""]
    bl.child_json(out)


def main(argv=None):
    ap = bl.parser(quick=True)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = bl.parse(ap, argv)
    if args.child:
        return child(args.child, args.runs)
    report = bl.Report(args.out)
    say = report.say
    if args.parent_tree:                                     # children first: this process has not opened the GPU yet
        res = bl.ab_children(__file__, bl.ROOT, args.parent_tree, args.ab_rounds, args.runs, timeout=300)
        say(f"## la_alignment_posteriors: this tree against the parent commit, fresh processes alternated, median of {args.runs} calls each (ms)")
        for key in res["this"][0]:
            for line in bl.against_parent_processes(key, [p[key] for p in res["this"]], [p[key] for p in res["parent"]]):
                say(line)
        say("")

    dev, lib = bl.open_gpu()
    from lyricalignment_amd.utils.alignment import spans_from_lines
    lines = QUICK_LINES if args.quick else LINES
    say(f"# confidences with optional lines on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after warm-up, "
        "device events, ms; boundary_window 2, no gamma output, skip_penalty 0")
    for (B, T, L), names in zip(QUICK if args.quick else SHAPES, leg_table(args.quick)):
        c, frames, plain = _plain(lib, dev, B, T, L, lines)
        skip_none = torch.full((B, L + 1), -1, dtype=torch.int32, device=dev)
        row = spans_from_lines(lines, [True] * len(lines)) + [-1] * (L - sum(lines))
        skip_all = bl.rows(row, B, dev)
        dp_s = bl.dp_leg(lib, "viterbi_spans", c, skip_all)          # the span DP's frames for the span lattice (once, untimed)
        bl.warm_up([("", dp_s)], 1)
        on_s = dp_s[1]["onset"]
        four_lines = bl.posterior_leg(lib, "alignment_posteriors_spans", c, (on_s, dp_s[1]["offset"]), skip_all)
        legs = list(zip(names, (plain, bl.posterior_leg(lib, "alignment_posteriors_spans", c, frames, skip_none), four_lines)))
        bl.warm_up(legs)
        assert bl.same_bits(plain[1], legs[1][1][1], bl.POSTERIOR_OUT), "no-span outputs differ"
        assert bl.ok(four_lines[1]) and bl.ok(dp_s[1])
        ends = [n for n, a in enumerate(row) if a >= 0]
        left_out = sorted({int(n) for n in (on_s < 0).nonzero()[:, 1].tolist()})
        ts = bl.alternated(legs, args.runs, warmup=0)
        stats = [bl.stat(ts[name]) for name in names]
        (mp, lp, hp), (mn, _, _), (ma, _, _) = stats
        say(f"## {B} clips x {T} frames x {L} labels (workspace {four_lines[0].workspace_bytes / 1e6:.1f} MB)")
        say(bl.timed(names[0], stats[0], 56))
        say(bl.timed(names[1], stats[1], 56) + f"   {mn / mp:5.2f} x   {1e3 * (mn - mp) / (2 * T):+.3f} us per step and sweep")
        say(bl.timed(names[2], stats[2], 56) + f"   {ma / mp:5.2f} x   {1e3 * (ma - mp) / (2 * T):+.3f} us per step and sweep")
        say(f"baseline's own spread (max - min) {hp - lp:.3f} ms; no-span outputs equal la_alignment_posteriors' bit for bit; labels the span DP "
            f"left out: {left_out}; span_skip_prob of clip 0 at the line ends {[round(float(four_lines[1]['span_skip'][0, n]), 4) for n in ends]}")
        say("")
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
