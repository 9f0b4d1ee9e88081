"""Cost of the confidences on the lattice with per-state frame windows (la_alignment_posteriors_windows) beside la_alignment_posteriors and
la_alignment_posteriors_spans; all three are instantiations of one kernel in csrc/la_posterior.hip.

    python tools/anchored_confidence_bench.py [--runs 30] [--quick] [--parent-lib <liblyricalign_hip.so of the parent commit>] [--out profiles/anchored_confidence.txt]

Two shapes on the synthetic emissions of tools/anchored_bench.py -- 32 clips x 1500 frames x 26 labels (four lines of 6 / 7 / 6 / 7 characters;
one wave) and one song of 5389 frames x 200 labels (four lines of 50; 8 waves); the emissions plant lines 1, 2 and 4.
Legs, alternated call by call (caller-owned buffers, no gamma output, boundary_window 2, device events around one call, a synchronise after each):
  * la_alignment_posteriors;
  * la_alignment_posteriors_spans without a span, and with the four lines optional;
  * la_alignment_posteriors_windows with every window [0, T) and a null skip_from: what the window instantiation costs when nothing is known;
  * la_alignment_posteriors_windows with one onset anchor per line (the line's first character within 1 s of where the unanchored DP put it);
  * la_alignment_posteriors_windows with those anchors and the four lines optional.
The DP that supplies each leg's onset / offset runs once, untimed.  With --parent-lib the parent commit's la_alignment_posteriors and
la_alignment_posteriors_spans (no span, four lines) run in the same alternation: each existing entry of this tree is placed against the
parent's own min .. max, and the all-open leg against the span-free la_alignment_posteriors_spans on the same inputs.
Every number is the median of `runs` calls after a warm-up; min .. max is printed next to it.  Before anything is timed the all-open outputs
are checked bit for bit against la_alignment_posteriors_spans', and every leg's status is LA_OK.
"""
from __future__ import annotations

import torch

import benchlib as bl

LEGS = ("la_alignment_posteriors", "la_alignment_posteriors_spans, no span", "la_alignment_posteriors_spans, four optional lines",
        "la_alignment_posteriors_windows, all windows open", "la_alignment_posteriors_windows, one onset anchor per line, +-1 s",
        "la_alignment_posteriors_windows, anchors + four optional lines")
PRESENT = [True, True, False, True]
SHAPES = [("32 clips x 1500 frames x 26 labels (1 wave)", 32, 1500, [6, 7, 6, 7]),
          ("1 song x 5389 frames x 200 labels (8 waves)", 1, 5389, [50, 50, 50, 50])]
QUICK = [("2 clips x 160 frames x 8 labels (1 wave)", 2, 160, [2, 2, 2, 2]), ("1 song x 400 frames x 40 labels (2 waves)", 1, 400, [10, 10, 10, 10])]
TOL_S = 1.0
DP_GATE_PERCENT = 5.7      # what the window gate cost the DP at 32 x 1500 x 26 (profiles/anchored_alignment.txt)


def leg_table(quick=False):
    """Per shape, the names the report gives the legs."""
    return [list(LEGS) for _ in (QUICK if quick else SHAPES)]


def main(argv=None):
    args = bl.parse(bl.parser(parent_lib=True, quick=True), argv)
    report = bl.Report(args.out)
    say = report.say
    dev, lib = bl.open_gpu()
    from lyricalignment_amd import ops
    from lyricalignment_amd.utils.alignment import spans_from_lines
    parent = bl.load_parent(args.parent_lib, ("alignment_posteriors", "alignment_posteriors_spans")) if args.parent_lib else None

    say(f"# confidences on the lattice with per-state frame windows on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls "
        f"after a warm-up of 3, legs alternated call by call, device events around one call, ms; boundary_window 2, no gamma output")
    for title, B, T, line_lengths in QUICK if args.quick else SHAPES:
        L = sum(line_lengths)
        c = bl.case(bl.planted(B, T, L, bl.sung_lines(line_lengths, PRESENT), B + T + L, dev), *bl.sheet(B, T, L, dev))    # lines 1, 2 and 4
        skip_none = torch.full((B, L + 1), -1, dtype=torch.int32, device=dev)
        skip_all = bl.rows(spans_from_lines(line_lengths, [True] * len(line_lengths)), B, dev)
        starts = bl.starts_of(line_lengths)

        # the DPs that supply onset / offset, once, untimed
        dp_plain = ops.viterbi_batch(*c[3:])
        dp_spans = ops.viterbi_spans_batch(*c[3:], skip_all, 0.0)
        win_open = bl.open_windows(B, T, L, dev)
        win_a = bl.anchored_windows(dp_plain[0], starts, T, L, TOL_S)
        win_s = bl.anchored_windows(dp_spans[0], starts, T, L, TOL_S)
        dp_anch = ops.viterbi_windows_batch(*c[3:], *win_a)
        dp_anch_s = ops.viterbi_windows_batch(*c[3:], *win_s, skip_all, 0.0)
        torch.cuda.synchronize()
        for dp in (dp_plain, dp_spans, dp_anch, dp_anch_s):
            assert int(dp[3].abs().sum()) == 0, "a DP leg is not LA_OK"

        def existing(lib_):
            return [bl.posterior_leg(lib_, "alignment_posteriors", c, dp_plain[:2]),
                    bl.posterior_leg(lib_, "alignment_posteriors_spans", c, dp_plain[:2], skip_none),
                    bl.posterior_leg(lib_, "alignment_posteriors_spans", c, dp_spans[:2], skip_all)]

        legs = list(zip(LEGS, existing(lib) + [bl.posterior_leg(lib, "alignment_posteriors_windows", c, dp_plain[:2], None, win_open),
                                               bl.posterior_leg(lib, "alignment_posteriors_windows", c, dp_anch[:2], None, win_a),
                                               bl.posterior_leg(lib, "alignment_posteriors_windows", c, dp_anch_s[:2], skip_all, win_s)]))
        if parent is not None:
            legs += [("parent commit: " + name, leg) for name, leg in zip(LEGS, existing(parent))]
        bl.warm_up(legs)
        outs = [out for _, (_, out) in legs]
        assert bl.same_bits(outs[1], outs[3], bl.SPAN_OUT), "all-open outputs differ from la_alignment_posteriors_spans'"
        assert bl.same_bits(outs[0], outs[1], bl.POSTERIOR_OUT), "span-free outputs differ from la_alignment_posteriors'"
        for name, (_, out) in legs:
            assert bl.ok(out), f"{name}: status not LA_OK"
        closed = float(((win_a[0] > 0) | (win_a[1] < T)).float().mean())
        wlp_a = (outs[4]["log_z"] - outs[0]["log_z"]).cpu()
        wlp_s = (outs[5]["log_z"] - outs[2]["log_z"]).cpu()
        stats = bl.stats_of(bl.alternated(legs, args.runs, warmup=0))
        say(f"## {title}")
        for name, st in stats.items():
            say(bl.timed(name, st, 70) + f"   {st[0] / stats[LEGS[0]][0]:5.2f} x la_alignment_posteriors")
        say(f"all-open outputs equal la_alignment_posteriors_spans' bit for bit; anchors narrow {100 * closed:.0f} % of the states' windows; every "
            f"status LA_OK; window_log_prob (windowed log_z - free log_z) of the anchored legs: {float(wlp_a.min()):.3f} .. {float(wlp_a.max()):.3f} "
            f"(anchors), {float(wlp_s.min()):.3f} .. {float(wlp_s.max()):.3f} (anchors + optional lines)")
        for i, j, what in ((3, 1, "all windows open against la_alignment_posteriors_spans, no span"),
                           (4, 1, "one onset anchor per line against la_alignment_posteriors_spans, no span"),
                           (5, 2, "anchors + four optional lines against la_alignment_posteriors_spans, four optional lines")):
            m, base = stats[LEGS[i]][0], stats[LEGS[j]][0]
            say(f"{what}: {m:.3f} against {base:.3f} ({100 * (m / base - 1):+.1f} %; the DP's gate measured +{DP_GATE_PERCENT} % all open)")
        for name in LEGS[:3] if parent is not None else ():
            say(bl.against_parent(name, stats[name], stats["parent commit: " + name]))
        say("")
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
