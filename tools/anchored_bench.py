"""Cost of the alignment DP with per-state frame windows (la_viterbi_windows_batch) beside la_viterbi_batch and
la_viterbi_spans_batch; all three are instantiations of one kernel in csrc/la_viterbi.hip.

    python tools/anchored_bench.py [--runs 30] [--quick] [--parent-lib <liblyricalign_hip.so of the parent commit>] [--out profiles/anchored_alignment.txt]

Two shapes on synthetic emissions -- 32 clips x 1500 frames x 26 labels (four lines of 6 / 7 / 6 / 7 characters; one wave, masks in LDS)
and one song of 5389 frames x 200 labels (four lines of 50; 8 waves, masks in the workspace); the emissions plant lines 1, 2 and 4.
Legs, alternated call by call (caller-owned buffers, device events around one call, a synchronise after each):
  * la_viterbi_batch;
  * la_viterbi_spans_batch without a span, and with the four lines optional;
  * la_viterbi_windows_batch with every window [0, T) and a null skip_from: what the window instantiation costs when nothing is known;
  * la_viterbi_windows_batch with one onset anchor per line (the line's first character within 1 s of where the unanchored DP put it);
  * la_viterbi_windows_batch with those anchors and the four lines optional.
With --parent-lib the parent commit's la_viterbi_batch and span-free la_viterbi_spans_batch run in the same alternation: the yardstick of
the all-open leg is the parent's span-free la_viterbi_spans_batch (inside its min .. max or not).
Every number is the median of `runs` calls after a warm-up; min .. max is printed next to it.  The all-open outputs are checked bit for
bit against la_viterbi_batch's, and every anchored leg's status is LA_OK, before anything is timed.
"""
from __future__ import annotations

import torch

import benchlib as bl

LEGS = ("la_viterbi_batch", "la_viterbi_spans_batch, no span", "la_viterbi_spans_batch, four optional lines",
        "la_viterbi_windows_batch, all windows open", "la_viterbi_windows_batch, one onset anchor per line, +-1 s",
        "la_viterbi_windows_batch, anchors + four optional lines")
PRESENT = [True, True, False, True]
SHAPES = [("32 clips x 1500 frames x 26 labels (1 wave, masks in LDS)", 32, 1500, [6, 7, 6, 7]),
          ("1 song x 5389 frames x 200 labels (8 waves, masks in the workspace)", 1, 5389, [50, 50, 50, 50])]
QUICK = [("2 clips x 160 frames x 8 labels (1 wave)", 2, 160, [2, 2, 2, 2]), ("1 song x 400 frames x 40 labels (2 waves)", 1, 400, [10, 10, 10, 10])]
TOL_S = 1.0


def leg_table(quick=False):
    """Per shape, the names the report gives the legs."""
    return [list(LEGS) for _ in (QUICK if quick else SHAPES)]


def main(argv=None):
    args = bl.parse(bl.parser(parent_lib=True, quick=True), argv)
    report = bl.Report(args.out)
    say = report.say
    dev, lib = bl.open_gpu()
    from lyricalignment_amd.utils.alignment import spans_from_lines
    parent = bl.load_parent(args.parent_lib, ("viterbi", "viterbi_spans")) if args.parent_lib else None

    say(f"# alignment DP with per-state frame windows on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a "
        f"warm-up of 3, legs alternated call by call, device events around one call, ms")
    for title, B, T, line_lengths in QUICK if args.quick else SHAPES:
        L = sum(line_lengths)
        c = bl.case(bl.planted(B, T, L, bl.sung_lines(line_lengths, PRESENT), B + T + L, dev), *bl.sheet(B, T, L, dev))    # lines 1, 2 and 4
        skip_none = torch.full((B, L + 1), -1, dtype=torch.int32, device=dev)
        skip_all = bl.rows(spans_from_lines(line_lengths, [True] * len(line_lengths)), B, dev)
        starts = bl.starts_of(line_lengths)

        legs = list(zip(LEGS, (bl.dp_leg(lib, "viterbi", c), bl.dp_leg(lib, "viterbi_spans", c, skip_none), bl.dp_leg(lib, "viterbi_spans", c, skip_all))))
        bl.warm_up(legs, 1)
        win_a = bl.anchored_windows(legs[0][1][1]["onset"], starts, T, L, TOL_S)
        win_s = bl.anchored_windows(legs[2][1][1]["onset"], starts, T, L, TOL_S)
        legs += list(zip(LEGS[3:], (bl.dp_leg(lib, "viterbi_windows", c, None, bl.open_windows(B, T, L, dev)),
                                    bl.dp_leg(lib, "viterbi_windows", c, None, win_a), bl.dp_leg(lib, "viterbi_windows", c, skip_all, win_s))))
        if parent is not None:
            legs += [("parent commit: " + LEGS[0], bl.dp_leg(parent, "viterbi", c)), ("parent commit: " + LEGS[1], bl.dp_leg(parent, "viterbi_spans", c, skip_none))]
        bl.warm_up(legs)
        outs = [out for _, (_, out) in legs]
        assert bl.same_bits(outs[0], outs[3], bl.DP_OUT), "all-open outputs differ from la_viterbi_batch"
        assert bl.same_bits(outs[0], outs[1], bl.DP_OUT), "span-free outputs differ from la_viterbi_batch"
        for name, (_, out) in legs:
            assert bl.ok(out), f"{name}: status not LA_OK"
        same = bl.same_bits(outs[2], outs[5], bl.DP_OUT)      # anchors laid around the span DP's own result
        closed = float(((win_a[0] > 0) | (win_a[1] < T)).float().mean())
        ts = bl.alternated(legs, args.runs, warmup=0)
        say(f"## {title}")
        stats = {name: bl.stat(t) for name, t in ts.items()}
        for name, st in stats.items():
            say(bl.timed(name, st, 62) + f"   {st[0] / stats[LEGS[0]][0]:5.2f} x la_viterbi_batch")
        say(f"all-open outputs equal la_viterbi_batch's bit for bit; anchors narrow {100 * closed:.0f} % of the states' windows; every status LA_OK; "
            f"anchored + optional result equals the unanchored one: {same}")
        if parent is not None:
            say(bl.against_parent(f"{LEGS[3]} beside the parent's span-free la_viterbi_spans_batch", stats[LEGS[3]], stats["parent commit: " + LEGS[1]]))
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
