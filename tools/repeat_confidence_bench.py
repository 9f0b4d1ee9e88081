"""Cost of the posteriors on the lattice with repeatable lyric lines (la_alignment_posteriors_repeats; the REP face of posterior_kernel in
csrc/la_posterior.hip) and what adding it did to the existing posterior entries.

    python tools/repeat_confidence_bench.py [--runs 30] [--quick] [--parent-lib <liblyricalign_hip.so of the parent commit>] [--out profiles/repeat_confidence.txt]

Two shapes on synthetic emissions -- 32 clips x 1500 frames x 26 labels (one wave) and one song of 5389 frames x 200 labels (8 waves) -- in
lines of 10 labels; the emissions plant the sheet with its second line (the chorus) sung twice.  Legs, alternated call by call
(caller-owned buffers, device events around one call, a synchronise after each; no gamma output):
  * the four existing entries: la_alignment_posteriors; la_alignment_posteriors_spans with every fourth line optional;
    la_alignment_posteriors_windows with every window open; la_alignment_posteriors_lattice with nothing given.  With --parent-lib the
    parent commit's same four legs run in the same alternation (outputs checked bit for bit against this build's) and every leg's median
    is reported against the parent's own min .. max of that leg: the project's noise yardstick;
  * la_alignment_posteriors_repeats with nothing repeatable and every window open (outputs checked bit for bit against
    la_alignment_posteriors_windows'), beside la_alignment_posteriors_windows of the same build;
  * la_alignment_posteriors_repeats with the chorus repeatable, with and without path_prob: reported;
  * the loops of a clip with a jump, old face beside new: la_alignment_posteriors_windows and la_alignment_posteriors_repeats (nothing
    repeatable) with the third line optional and every window open (outputs checked bit for bit): reported.
Every posterior leg is asked about the onset / offset (and path) that la_viterbi_repeats_batch reports for its lattice.  Every number is
the median of `runs` calls after a warm-up; min .. max is printed next to it.
"""
from __future__ import annotations

import torch

import benchlib as bl

EXISTING = ("la_alignment_posteriors", "la_alignment_posteriors_spans, every fourth line optional",
            "la_alignment_posteriors_windows, all windows open", "la_alignment_posteriors_lattice, nothing given")
NEW = ("la_alignment_posteriors_repeats, nothing repeatable, all windows open", "la_alignment_posteriors_repeats, one repeatable chorus",
       "la_alignment_posteriors_repeats, one repeatable chorus, with path_prob",
       "la_alignment_posteriors_windows, the third line optional, all windows open",
       "la_alignment_posteriors_repeats, the third line optional, nothing repeatable, all windows open")
STEMS = ("alignment_posteriors", "alignment_posteriors_spans", "alignment_posteriors_windows", "alignment_posteriors_lattice")
SHAPES = [("32 clips x 1500 frames x 26 labels (1 wave)", 32, 1500, 26, 10), ("1 song x 5389 frames x 200 labels (8 waves)", 1, 5389, 200, 10)]
# the chorus is sung twice: 50 planted labels of the 40 need 4 * 101 frames
QUICK = [("2 clips x 160 frames x 8 labels (1 wave)",) + bl.QUICK_ONE_WAVE, ("1 song x 408 frames x 40 labels (2 waves)", 1, 408, 40, 10)]


def leg_table(quick=False):
    """Per shape, the names the report gives the legs."""
    return [list(EXISTING + NEW) for _ in (QUICK if quick else SHAPES)]


def main(argv=None):
    args = bl.parse(bl.parser(parent_lib=True, quick=True), argv)
    report = bl.Report(args.out)
    say = report.say
    dev, lib = bl.open_gpu()
    from lyricalignment_amd import ops
    from lyricalignment_amd.utils.alignment import repeats_from_lines, spans_from_lines
    parent = bl.load_parent(args.parent_lib, STEMS) if args.parent_lib else None

    say(f"# posteriors on the lattice with repeatable lines on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a "
        f"warm-up of 3, legs alternated call by call, device events around one call, ms")
    for title, B, T, L, line in QUICK if args.quick else SHAPES:
        lengths, starts = bl.lines_of(L, line)
        c = bl.case(bl.planted(B, T, L, bl.sung_lines(lengths, [2 if i == 1 else 1 for i in range(len(lengths))]), B + T + L, dev),
                    *bl.sheet(B, T, L, dev))
        sheet = bl.rows(spans_from_lines(lengths, [i % 4 == 3 for i in range(len(lengths))]), B, dev)
        verse = bl.rows(spans_from_lines(lengths, [i == 2 for i in range(len(lengths))]), B, dev)
        chorus = bl.rows(repeats_from_lines(lengths, [i == 1 for i in range(len(lengths))]), B, dev)
        win = bl.open_windows(B, T, L, dev)

        def leg(lib_, stem, skip=None, windows=None, repeat=None, with_path=False):
            """-> (call, outputs); every leg asks about its own lattice's DP result"""
            dp = ops.viterbi_repeats_batch(*c[3:], skip, 0.0, *(windows or (None, None)), repeat, 0.0)
            assert int(dp[3].abs().sum()) == 0
            return bl.posterior_leg(lib_, stem, c, dp[:2], skip, windows, repeat, dp[4] if with_path else None)

        def existing(lib_):
            return [leg(lib_, STEMS[0]), leg(lib_, STEMS[1], sheet), leg(lib_, STEMS[2], None, win), leg(lib_, STEMS[3])]

        legs = list(zip(EXISTING, existing(lib)))
        legs += list(zip(NEW, [leg(lib, "alignment_posteriors_repeats", None, win), leg(lib, "alignment_posteriors_repeats", None, None, chorus),
                               leg(lib, "alignment_posteriors_repeats", None, None, chorus, True),
                               leg(lib, "alignment_posteriors_windows", verse, win), leg(lib, "alignment_posteriors_repeats", verse, win)]))
        if parent is not None:
            legs += [("parent commit: " + name, l) for name, l in zip(EXISTING, existing(parent))]
        bl.warm_up(legs)
        outs = [out for _, (_, out) in legs]
        for name, (_, out) in legs:
            assert bl.ok(out), f"{name}: status not LA_OK"
        assert bl.same_bits(outs[2], outs[4], bl.SPAN_OUT), "nothing repeatable differs from la_alignment_posteriors_windows"
        assert int(outs[4]["repeat_count"].abs().sum()) == 0
        assert bl.same_bits(outs[7], outs[8], bl.SPAN_OUT), "one optional line: the new face differs from the old"
        for i in range(4) if parent is not None else ():
            assert bl.same_bits(outs[i], outs[9 + i], bl.SPAN_OUT if i else bl.POSTERIOR_OUT), f"{legs[i][0]}: outputs differ from the parent commit's"
        stats = bl.stats_of(bl.alternated(legs, args.runs, warmup=0))
        say(f"## {title}")
        for name, st in stats.items():
            say(bl.timed(name, st, 86))
        rc, vis = outs[5]["repeat_count"][0], outs[5]["present"][0]
        say(f"clip 0 with the chorus repeatable: repeat_count of the chorus {float(rc[starts[1]]):.4f}, visits of its first label "
            f"{float(vis[starts[1]]):.4f}, of the label after it {float(vis[starts[2]]):.4f}; nothing-repeatable outputs equal "
            f"la_alignment_posteriors_windows' bit for bit; every status LA_OK")
        m, base = stats[NEW[0]][0], stats[EXISTING[2]][0]
        say(f"{NEW[0]}: {m:.3f} beside {EXISTING[2]} {base:.3f} of the same build ({100 * (m / base - 1):+.1f} %)")
        m, base2 = stats[NEW[4]][0], stats[NEW[3]][0]
        say(f"{NEW[4]}: {m:.3f} beside {NEW[3]} {base2:.3f} ({100 * (m / base2 - 1):+.1f} %), outputs equal bit for bit")
        for name in NEW[1:3]:
            say(f"{name}: {stats[name][0]:.3f} ({100 * (stats[name][0] / base - 1):+.1f} % of {EXISTING[2]})")
        for name in EXISTING if parent is not None else ():
            say(bl.against_parent(name, stats[name], stats["parent commit: " + name]))
        say()
        del legs, outs, c
        torch.cuda.empty_cache()
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
