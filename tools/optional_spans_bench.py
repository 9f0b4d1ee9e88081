"""Cost of the alignment DP with optional lyric lines (la_viterbi_spans_batch) beside la_viterbi_batch; both are
instantiations of one kernel in csrc/la_viterbi.hip, without and with the span code.

    python tools/optional_spans_bench.py [--runs 30] [--quick] [--out profiles/optional_spans.txt]

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

import torch

import benchlib as bl

LEGS = ("la_viterbi_batch (baseline)", "la_viterbi_spans_batch, no spans", "la_viterbi_spans_batch, lines of {} optional")
FULL, QUICK = (32, 1500, [6, 7, 6, 7]), (2, 160, [2, 2, 2, 2])
PRESENT = [True, True, False, True]


def leg_table(quick=False):
    """Per shape, the names the report gives the legs."""
    return [[name.format("/".join(map(str, (QUICK if quick else FULL)[2]))) for name in LEGS]]


def main(argv=None):
    args = bl.parse(bl.parser(quick=True), argv)
    report = bl.Report(args.out)
    say = report.say
    dev, lib = bl.open_gpu()
    from lyricalignment_amd.utils.alignment import spans_from_lines
    B, T, LINES = QUICK if args.quick else FULL
    L = sum(LINES)
    c = bl.case(bl.planted(B, T, L, bl.sung_lines(LINES, PRESENT), B + T + L, dev), *bl.sheet(B, T, L, dev))     # lines 1, 2 and 4 are sung
    skip_none = torch.full((B, L + 1), -1, dtype=torch.int32, device=dev)
    skip_all = bl.rows(spans_from_lines(LINES, [True] * len(LINES)), B, dev)
    names = leg_table(args.quick)[0]
    legs = list(zip(names, (bl.dp_leg(lib, "viterbi", c), bl.dp_leg(lib, "viterbi_spans", c, skip_none), bl.dp_leg(lib, "viterbi_spans", c, skip_all))))
    bl.warm_up(legs)
    out_v, out_n, out_a = (out for _, (_, out) in legs)
    assert bl.same_bits(out_v, out_n, bl.DP_OUT), "no-span outputs differ from la_viterbi_batch"
    assert bl.ok(out_a)
    left_out = sorted({int(n) for n in (out_a["onset"] < 0).nonzero()[:, 1].tolist()})
    ts = bl.alternated(legs, args.runs, warmup=0)
    stats = [bl.stat(ts[name]) for name in names]
    (mv, lv, hv), (mn, _, _), (ma, _, _) = stats
    say(f"# alignment DP with optional lines on {torch.cuda.get_device_name(0)}; {B} clips x {T} frames x {L} labels, median (min .. max) of "
        f"{args.runs} calls after warm-up, device events, ms")
    say(bl.timed(names[0], stats[0], 49, 7))
    say(bl.timed(names[1], stats[1], 49, 7) + f"   {mn / mv:5.2f} x   {1e3 * (mn - mv) / T:+.3f} us per frame")
    say(bl.timed(names[2], stats[2], 49, 7) + f"   {ma / mv:5.2f} x   {1e3 * (ma - mv) / T:+.3f} us per frame")
    say(f"baseline's own spread (max - min) {hv - lv:.3f} ms; no-span outputs equal la_viterbi_batch's bit for bit; labels left out with the "
        f"spans: {left_out}")
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
