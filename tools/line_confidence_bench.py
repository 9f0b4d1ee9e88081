"""Cost of the confidence for free line order (la_alignment_posteriors_lines; csrc/la_line_posterior.hip) beside the entries it stands next to.

    python tools/line_confidence_bench.py [--runs 30] [--quick] [--parent-lib <liblyricalign_hip.so of the parent commit>]
        [--out profiles/line_confidence.txt]

Synthetic emissions as tools/line_order_bench.py plants them (the sheet with its second line sung twice): 32 clips x 1500 frames x 26 labels
in 4 lines (one wave), one song of 12000 frames x 800 labels with 10 and with 100 lines (2 states per thread) and one of 12000 x 2500 in
250 lines (8 states per thread).  Legs on the same emissions, alternated call by call (caller-owned buffers, device events around one
call, a synchronise after each):
  * la_viterbi_lines_batch, the DP whose onset / offset / path the sweep is asked about;
  * la_alignment_posteriors_song with the whole sheet as one repeat span (the one-line face of the same lattice), on the frames and the path
    of la_viterbi_repeats_batch with that span;
  * la_alignment_posteriors_lines (line_jump_penalty 1), once per line count.
Every number is the median of `runs` calls after a warm-up; min .. max is printed next to it.  The numbers are recorded, not gated.  With
--parent-lib the parent commit's legs run in the same alternation: every output is compared byte for byte and every leg's median is reported
against the parent's min .. max.
"""
from __future__ import annotations

import torch

import benchlib as bl
from line_order_bench import flags, lengths_of, lines_leg

SWEEP = "la_alignment_posteriors_lines"
# title, B, T, L, the line counts timed on the same emissions (the first one plants the performance)
SHAPES = [("32 clips x 1500 frames x 26 labels (1 wave)", 32, 1500, 26, (4,)),
          ("1 song x 12000 frames x 800 labels (2 states per thread)", 1, 12000, 800, (10, 100)),
          ("1 song x 12000 frames x 2500 labels (8 states per thread)", 1, 12000, 2500, (250,))]
QUICK = [("2 clips x 160 frames x 8 labels (1 wave)",) + bl.QUICK_ONE_WAVE[:3] + ((4,),),
         ("1 song x 408 frames x 40 labels (2 waves)", 1, 408, 40, (2, 8)),
         ("1 song x 4400 frames x 520 labels (2 states per thread)",) + bl.QUICK_STRIP[:3] + ((52,),)]


def sweep_leg(lib, c, line_start, frames, path, penalty=1.0):
    """la_alignment_posteriors_lines of `lib` on `c`, asked about the DP's frames and path -> (fn, outputs)."""
    return bl.posterior_leg(lib, "alignment_posteriors_lines", c, frames, path=path, row=line_start, scalar=float(penalty))


def main(argv=None):
    args = bl.parse(bl.parser(parent_lib=True, quick=True), argv)
    report = bl.Report(args.out)
    say = report.say
    dev, lib = bl.open_gpu()
    parent = bl.load_parent(args.parent_lib, ("viterbi_repeats", "alignment_posteriors_song", "viterbi_lines", "alignment_posteriors_lines")) \
        if args.parent_lib else None

    say(f"# confidence for free line order on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a warm-up of 3, "
        f"legs alternated call by call, device events around one call, ms")
    for title, B, T, L, line_counts in QUICK if args.quick else SHAPES:
        lengths = lengths_of(L, line_counts[0])
        c = bl.case(bl.planted(B, T, L, bl.sung_lines(lengths, [2 if i == 1 else 1 for i in range(len(lengths))]), B + T + L, dev),
                    *bl.sheet(B, T, L, dev))
        whole = bl.rows([L] + [-1] * (L - 1), B, dev)                      # the whole sheet as one repeat span

        def build(lib_):
            rep_dp = bl.dp_leg(lib_, "viterbi_repeats", c, None, None, whole)
            rep_dp[0]()
            legs = [("la_alignment_posteriors_song, the sheet one repeat span", bl.posterior_leg(
                lib_, "alignment_posteriors_song", c, (rep_dp[1]["onset"], rep_dp[1]["offset"]), repeat=whole, path=rep_dp[1]["path"]))]
            for n in line_counts:
                ls = flags(L, n, B, dev)
                dp = lines_leg(lib_, c, ls)
                dp[0]()
                torch.cuda.synchronize()
                assert bl.ok(dp[1]), f"la_viterbi_lines_batch, {n} lines: status not LA_OK"
                legs.append((f"la_viterbi_lines_batch, {n} lines", dp))
                legs.append((f"{SWEEP}, {n} lines", sweep_leg(lib_, c, ls, (dp[1]["onset"], dp[1]["offset"]), dp[1]["path"])))
            return legs
        legs = bl.with_parent(build, lib, parent)
        bl.warm_up(legs)
        for name, (_, out) in legs:
            assert bl.ok(out), f"{name}: status not LA_OK"
        stats = bl.stats_of(bl.alternated(legs, args.runs, warmup=0))
        say(f"## {title}")
        for name, st in stats.items():
            say(bl.timed(name, st, 60))
        for n in line_counts:
            fn, out = dict(legs)[f"{SWEEP}, {n} lines"]
            m = stats[f"{SWEEP}, {n} lines"][0]
            vis = out["visits"][0].double()
            say(f"{n} lines: workspace {fn.workspace_bytes} bytes; log_z {out['log_z'][0].item():.6f}; expected visits of clip 0 in all "
                f"{vis.sum().item():.3f} over {L} labels, largest {vis.max().item():.3f}; sweep {m:.3f} = "
                f"{m / stats[f'la_viterbi_lines_batch, {n} lines'][0]:.2f} x its DP, {m / stats[legs[0][0]][0]:.2f} x la_alignment_posteriors_song")
        if len(line_counts) == 2:
            a, b = (stats[f"{SWEEP}, {n} lines"] for n in line_counts)
            say(f"{line_counts[0]} lines {a[0]:.3f} ({a[1]:.3f} .. {a[2]:.3f}) against {line_counts[1]} lines {b[0]:.3f} ({b[1]:.3f} .. {b[2]:.3f}): "
                f"{100 * (b[0] / a[0] - 1):+.1f} %")
        bl.say_against_parent(say, legs, stats)
        say()
        del legs, c
        torch.cuda.empty_cache()
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
