"""Cost of the alignment DP with a minimum character duration (la_viterbi_min_duration_batch; csrc/la_min_duration.hip) beside
la_viterbi_batch on the same build.

    python tools/min_duration_bench.py [--runs 30] [--quick] [--parent-lib <liblyricalign_hip.so of the parent commit>] [--out profiles/min_duration.txt]

Four shapes on synthetic emissions -- 32 clips x 1500 frames x 26 labels (one wave), one song of 5389 frames x 200 labels (8 waves), one
of 12000 x 800 (2 states per thread) and one of 12000 x 2500 (8 states per thread); the emissions plant the sheet sung straight through.
Legs, alternated call by call (caller-owned buffers, device events around one call, a synchronise after each):
  * la_viterbi_batch, the yardstick: its code is untouched by the minimum duration;
  * la_viterbi_min_duration_batch with every floor 1, 3 and 8 frames, each with max_min_frames = that floor (chain depths 2, 4 and 8), and
    with every floor 1 at max_min_frames = 8: the deepest chain doing the shallowest work.  Where the floor times the labels would not fit
    into nine tenths of the frames (8 x 2500 > 12000) only the first K labels get the floor and the rest 1; K is reported.
The floor-1 outputs are compared with la_viterbi_batch's and the report says whether they are the same bits; under a floor the report
gives the shortest character of clip 0.  Every number is the median of `runs` calls after a warm-up; min .. max is printed next to it.
The times are recorded, not gated.  With --parent-lib the parent commit's legs run in the same alternation: every output is compared byte for
byte and every leg's median is reported against the parent's min .. max.
"""
from __future__ import annotations

import torch

import benchlib as bl

# title, B, T, L
SHAPES = [("32 clips x 1500 frames x 26 labels (1 wave)", 32, 1500, 26),
          ("1 song x 5389 frames x 200 labels (8 waves)", 1, 5389, 200),
          ("1 song x 12000 frames x 800 labels (2 states per thread)", 1, 12000, 800),
          ("1 song x 12000 frames x 2500 labels (8 states per thread)", 1, 12000, 2500)]
QUICK = [("2 clips x 160 frames x 8 labels (1 wave)",) + bl.QUICK_ONE_WAVE[:3],
         ("1 song x 400 frames x 40 labels (2 waves)",) + bl.QUICK_MULTI_WAVE[:3],
         ("1 song x 4400 frames x 520 labels (2 states per thread)",) + bl.QUICK_STRIP[:3]]
# the floor of every label, max_min_frames
FLOORS = [(1, 1), (3, 3), (8, 8), (1, 8)]


def floor_leg(lib, c, floor, max_min_frames):
    """la_viterbi_min_duration_batch of `lib` on `c` with one floor for every label that fits (floored_labels) -> (fn, outputs)."""
    K = floored_labels(c.T, c.L, floor)
    return bl.dp_leg(lib, "viterbi_min_duration", c, row=bl.rows([floor] * K + [1] * (c.L - K), c.B, c.em.device), scalar=int(max_min_frames))


def floored_labels(T, L, floor):
    """How many of the L labels get the floor: all, or as many as leave the tight path inside nine tenths of the T frames."""
    return L if floor == 1 else min(L, max(0, (9 * T // 10 - L) // (floor - 1)))


def name_of(floor, max_min_frames):
    return f"la_viterbi_min_duration_batch, floor {floor}, max_min_frames {max_min_frames}"


def main(argv=None):
    args = bl.parse(bl.parser(parent_lib=True, quick=True), argv)
    report = bl.Report(args.out)
    say = report.say
    dev, lib = bl.open_gpu()
    parent = bl.load_parent(args.parent_lib, ("viterbi", "viterbi_min_duration")) if args.parent_lib else None

    say(f"# alignment DP with a minimum character duration on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after "
        f"a warm-up of 3, legs alternated call by call, device events around one call, ms")
    for title, B, T, L in QUICK if args.quick else SHAPES:
        c = bl.case(bl.planted(B, T, L, list(range(L)), B + T + L, dev), *bl.sheet(B, T, L, dev))
        legs = bl.with_parent(lambda lib_: [("la_viterbi_batch", bl.dp_leg(lib_, "viterbi", c))] + [(name_of(*f), floor_leg(lib_, c, *f)) for f in FLOORS],
                              lib, parent)
        bl.warm_up(legs)
        for name, (_, out) in legs:
            assert bl.ok(out), f"{name}: status not LA_OK"
        plain = legs[0][1][1]
        same = [bl.same_bits(plain, legs[i][1][1], ("onset", "offset", "score", "status")) for i in (1, 4)]
        shortest = {f: int((legs[1 + i][1][1]["offset"][0] - legs[1 + i][1][1]["onset"][0]).min()) for i, f in enumerate(FLOORS)}
        plain_shortest = int((plain["offset"][0] - plain["onset"][0]).min())
        stats = bl.stats_of(bl.alternated(legs, args.runs, warmup=0))
        say(f"## {title}")
        width = max(len(name) for name in stats)
        for name, st in stats.items():
            say(bl.timed(name, st, width))
        say(f"workspace of la_viterbi_min_duration_batch: {legs[1][1][0].workspace_bytes} bytes; every status LA_OK; floor 1 gives "
            f"{'the bits of' if all(same) else 'OTHER bits than'} la_viterbi_batch at both depths; shortest character of clip 0: "
            f"{plain_shortest} frames plain, " + ", ".join(f"{v} under {name_of(*f).split(', ', 1)[1]}" for f, v in shortest.items()))
        say("labels under the floor: " + ", ".join(f"{floored_labels(T, L, f[0])} of {L} at floor {f[0]}" for f in FLOORS[:3]))
        base = stats["la_viterbi_batch"][0]
        for f in FLOORS:
            m = stats[name_of(*f)][0]
            say(f"floor {f[0]} at max_min_frames {f[1]}: {m:.3f} beside la_viterbi_batch {base:.3f} ({100 * (m / base - 1):+.1f} %)")
        a, b = stats[name_of(1, 1)], stats[name_of(1, 8)]
        say(f"chain depth 2 {a[0]:.3f} ({a[1]:.3f} .. {a[2]:.3f}) against depth 8 {b[0]:.3f} ({b[1]:.3f} .. {b[2]:.3f}) at floor 1: "
            f"{100 * (b[0] / a[0] - 1):+.1f} %")
        bl.say_against_parent(say, legs, stats)
        say()
        del legs, c
        torch.cuda.empty_cache()
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
