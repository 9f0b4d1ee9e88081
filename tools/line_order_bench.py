"""Cost of the alignment DP with free line order (la_viterbi_lines_batch; csrc/la_line_order.hip) beside the entries it stands next to.

    python tools/line_order_bench.py [--runs 30] [--quick] [--parent-lib <liblyricalign_hip.so of the parent commit>] [--out profiles/line_order.txt]

Four shapes on synthetic emissions -- 32 clips x 1500 frames x 26 labels in 4 lines (one wave), one song of 5389 frames x 200 labels (8
waves), one of 12000 x 800 in 60 lines (2 states per thread) and one of 12000 x 2500 (8 states per thread); the emissions plant the sheet
with its second line (the chorus) sung twice.  Legs, alternated call by call (caller-owned buffers, device events around one call, a
synchronise after each):
  * la_viterbi_batch;
  * la_viterbi_repeats_batch with nothing repeatable, and with the chorus repeatable;
  * la_viterbi_lines_batch on the same sheet with its line breaks (line_jump_penalty 1); the visits on its reported path of clip 0 are
    compared with those of la_viterbi_repeats_batch with the chorus repeatable, and the report says whether they are the same;
  * at 12000 x 800 also la_viterbi_lines_batch with 10 lines and with 100 lines: the hub's work per frame does not depend on the number
    of lines, so the two should be equal; what is measured is reported.
Every number is the median of `runs` calls after a warm-up; min .. max is printed next to it.  With --parent-lib the parent commit's legs run
in the same alternation: every output is compared byte for byte and every leg's median is reported against the parent's min .. max.
"""
from __future__ import annotations

import torch

import benchlib as bl

LEGS = ("la_viterbi_batch", "la_viterbi_repeats_batch, nothing repeatable", "la_viterbi_repeats_batch, one repeatable chorus",
        "la_viterbi_lines_batch")
# title, B, T, L, lines, the further line counts timed on the same emissions
SHAPES = [("32 clips x 1500 frames x 26 labels in 4 lines (1 wave)", 32, 1500, 26, 4, ()),
          ("1 song x 5389 frames x 200 labels in 20 lines (8 waves)", 1, 5389, 200, 20, ()),
          ("1 song x 12000 frames x 800 labels in 60 lines (2 states per thread)", 1, 12000, 800, 60, (10, 100)),
          ("1 song x 12000 frames x 2500 labels in 250 lines (8 states per thread)", 1, 12000, 2500, 250, ())]
QUICK = [("2 clips x 160 frames x 8 labels in 4 lines (1 wave)",) + bl.QUICK_ONE_WAVE[:3] + (4, ()),
         ("1 song x 408 frames x 40 labels in 4 lines (2 waves)", 1, 408, 40, 4, (2, 8)),
         ("1 song x 4400 frames x 520 labels in 52 lines (2 states per thread)",) + bl.QUICK_STRIP[:3] + (52, ())]


def lengths_of(L, n_lines):
    """L labels in n_lines lines of (nearly) equal length."""
    return [(i + 1) * L // n_lines - i * L // n_lines for i in range(n_lines)]


def flags(L, n_lines, B, dev):
    """-> line_start [B, L] int32 of that sheet."""
    starts = set(bl.starts_of(lengths_of(L, n_lines)))
    return bl.rows([1 if n in starts else 0 for n in range(L)], B, dev)


def lines_leg(lib, c, line_start, penalty=1.0):
    """la_viterbi_lines_batch of `lib` on `c` -> (fn, outputs)."""
    return bl.dp_leg(lib, "viterbi_lines", c, row=line_start, scalar=float(penalty))


def visits_of(out):
    """The labels visited on the reported path of clip 0, in time order."""
    p = out["path"][0].cpu()
    odd = p[p % 2 == 1]
    keep = torch.ones_like(odd, dtype=torch.bool)
    keep[1:] = odd[1:] != odd[:-1]
    return (odd[keep] // 2).tolist()


def main(argv=None):
    args = bl.parse(bl.parser(parent_lib=True, quick=True), argv)
    report = bl.Report(args.out)
    say = report.say
    dev, lib = bl.open_gpu()
    parent = bl.load_parent(args.parent_lib, ("viterbi", "viterbi_repeats", "viterbi_lines")) if args.parent_lib else None
    from lyricalignment_amd.utils.alignment import repeats_from_lines

    say(f"# alignment DP with free line order on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a warm-up "
        f"of 3, legs alternated call by call, device events around one call, ms")
    for title, B, T, L, n_lines, more in QUICK if args.quick else SHAPES:
        lengths = lengths_of(L, n_lines)
        c = bl.case(bl.planted(B, T, L, bl.sung_lines(lengths, [2 if i == 1 else 1 for i in range(len(lengths))]), B + T + L, dev),
                    *bl.sheet(B, T, L, dev))
        chorus = bl.rows(repeats_from_lines(lengths, [i == 1 for i in range(len(lengths))]), B, dev)
        legs = bl.with_parent(lambda lib_: list(zip(LEGS, [
            bl.dp_leg(lib_, "viterbi", c), bl.dp_leg(lib_, "viterbi_repeats", c), bl.dp_leg(lib_, "viterbi_repeats", c, None, None, chorus),
            lines_leg(lib_, c, flags(L, n_lines, B, dev))])) + [(f"la_viterbi_lines_batch, {n} lines", lines_leg(lib_, c, flags(L, n, B, dev)))
                                                               for n in more], lib, parent)
        bl.warm_up(legs)
        for name, (_, out) in legs:
            assert bl.ok(out), f"{name}: status not LA_OK"
        sung, free = visits_of(legs[2][1][1]), visits_of(legs[3][1][1])
        stats = bl.stats_of(bl.alternated(legs, args.runs, warmup=0))
        say(f"## {title}")
        for name, st in stats.items():
            say(bl.timed(name, st, 52))
        say(f"workspace of la_viterbi_lines_batch: {legs[3][1][0].workspace_bytes} bytes; visits on the reported path of clip 0: {len(free)} "
            f"({L} labels on the sheet), {'the same labels as' if sung == free else 'OTHER labels than'} la_viterbi_repeats_batch's with the chorus "
            f"repeatable ({len(sung)}); every status LA_OK")
        m = stats[LEGS[3]][0]
        for name in LEGS[:3]:
            say(f"viterbi_lines {m:.3f} beside {name} {stats[name][0]:.3f} ({100 * (m / stats[name][0] - 1):+.1f} %)")
        if more:
            a, b = (stats[f"la_viterbi_lines_batch, {n} lines"] for n in more)
            say(f"{more[0]} lines {a[0]:.3f} ({a[1]:.3f} .. {a[2]:.3f}) against {more[1]} lines {b[0]:.3f} ({b[1]:.3f} .. {b[2]:.3f}): "
                f"{100 * (b[0] / a[0] - 1):+.1f} %")
        bl.say_against_parent(say, legs, stats)
        say()
        del legs, c
        torch.cuda.empty_cache()
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
