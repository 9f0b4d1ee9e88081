"""Cost of the alignment DP with repeatable lyric lines (la_viterbi_repeats_batch; csrc/la_viterbi.hip) and what adding it did to the
existing entries.

    python tools/repeat_lattice_bench.py [--runs 30] [--quick] [--parent-lib <liblyricalign_hip.so of the parent commit>] [--out profiles/repeat_lattice.txt]

Four shapes on synthetic emissions -- 32 clips x 1500 frames x 26 labels (one wave), one song of 5389 frames x 200 labels (8 waves), one of
12000 x 800 (2 states per thread) and one of 12000 x 2500 (8 states per thread) -- all in lines of 10 labels; the emissions plant the sheet
with its second line (the chorus) sung twice.  Legs, alternated call by call (caller-owned buffers, device events around one call, a
synchronise after each):
  * the existing entries: la_viterbi_batch; la_viterbi_lattice_batch with nothing given, with every fourth line optional, and with every
    window open.  With --parent-lib the parent commit's same four legs run in the same alternation (outputs checked bit for bit against this
    build's) and every leg's median is reported against the parent's own min .. max of that leg: the project's noise yardstick.  A leg
    outside it is reported with its excess;
  * la_viterbi_repeats_batch with nothing given (outputs checked bit for bit against la_viterbi_lattice_batch's), beside
    la_viterbi_lattice_batch of the same build;
  * la_viterbi_repeats_batch with the chorus repeatable, and with a repeat span over chorus .. verse plus that verse optional: reported.
Every number is the median of `runs` calls after a warm-up; min .. max is printed next to it.
"""
from __future__ import annotations

import torch

import benchlib as bl

EXISTING = ("la_viterbi_batch", "la_viterbi_lattice_batch, nothing given", "la_viterbi_lattice_batch, every fourth line optional",
            "la_viterbi_lattice_batch, all windows open")
NEW = ("la_viterbi_repeats_batch, nothing given", "la_viterbi_repeats_batch, one repeatable chorus",
       "la_viterbi_repeats_batch, repeat span chorus .. verse + the verse optional")
SHAPES = [("32 clips x 1500 frames x 26 labels (1 wave, masks in LDS)", 32, 1500, 26, 10),
          ("1 song x 5389 frames x 200 labels (8 waves)", 1, 5389, 200, 10),
          ("1 song x 12000 frames x 800 labels (2 states per thread)", 1, 12000, 800, 10),
          ("1 song x 12000 frames x 2500 labels (8 states per thread)", 1, 12000, 2500, 10)]
# the chorus is sung twice: 50 planted labels of the 40 need 4 * 101 frames
QUICK = [("2 clips x 160 frames x 8 labels (1 wave)",) + bl.QUICK_ONE_WAVE, ("1 song x 408 frames x 40 labels (2 waves)", 1, 408, 40, 10),
         ("1 song x 4400 frames x 520 labels (2 states per thread)",) + bl.QUICK_STRIP]


def leg_table(quick=False):
    """Per shape, the names the report gives the legs."""
    return [list(EXISTING + NEW) for _ in (QUICK if quick else SHAPES)]


def main(argv=None):
    args = bl.parse(bl.parser(parent_lib=True, quick=True), argv)
    report = bl.Report(args.out)
    say = report.say
    dev, lib = bl.open_gpu()
    from lyricalignment_amd.utils.alignment import repeats_from_lines, spans_from_lines
    parent = bl.load_parent(args.parent_lib, ("viterbi", "viterbi_lattice")) if args.parent_lib else None

    say(f"# alignment DP with repeatable lines on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a warm-up "
        f"of 3, legs alternated call by call, device events around one call, ms")
    for title, B, T, L, line in QUICK if args.quick else SHAPES:
        lengths, starts = bl.lines_of(L, line)
        c = bl.case(bl.planted(B, T, L, bl.sung_lines(lengths, [2 if i == 1 else 1 for i in range(len(lengths))]), B + T + L, dev),
                    *bl.sheet(B, T, L, dev))
        sheet = bl.rows(spans_from_lines(lengths, [i % 4 == 3 for i in range(len(lengths))]), B, dev)
        verse = bl.rows(spans_from_lines(lengths, [i == 2 for i in range(len(lengths))]), B, dev)
        chorus = bl.rows(repeats_from_lines(lengths, [i == 1 for i in range(len(lengths))]), B, dev)
        both = chorus.clone()
        both[:, starts[1]] = starts[2] + lengths[2]                        # the repeat span runs over chorus .. verse
        win = bl.open_windows(B, T, L, dev)

        def existing(lib_):
            return [bl.dp_leg(lib_, "viterbi", c), bl.dp_leg(lib_, "viterbi_lattice", c), bl.dp_leg(lib_, "viterbi_lattice", c, sheet),
                    bl.dp_leg(lib_, "viterbi_lattice", c, None, win)]

        legs = list(zip(EXISTING, existing(lib)))
        legs += list(zip(NEW, [bl.dp_leg(lib, "viterbi_repeats", c), bl.dp_leg(lib, "viterbi_repeats", c, None, None, chorus),
                               bl.dp_leg(lib, "viterbi_repeats", c, verse, None, both)]))
        if parent is not None:
            legs += [("parent commit: " + name, leg) for name, leg in zip(EXISTING, existing(parent))]
        bl.warm_up(legs, 1)
        outs = [out for _, (_, out) in legs]
        assert bl.same_bits(outs[1], outs[4], bl.DP_OUT), "la_viterbi_repeats_batch with nothing given differs from la_viterbi_lattice_batch"
        for i in range(4) if parent is not None else ():
            assert bl.same_bits(outs[i], outs[7 + i], bl.DP_OUT), f"{legs[i][0]}: outputs differ from the parent commit's"
        visits = []
        for i in (4, 5, 6):
            p = outs[i]["path"][0].cpu()
            odd = p[(p % 2 == 1)]
            visits.append(int((odd[1:] != odd[:-1]).sum()) + 1)
        bl.warm_up(legs)
        for name, (_, out) in legs:
            assert bl.ok(out), f"{name}: status not LA_OK"
        stats = bl.stats_of(bl.alternated(legs, args.runs, warmup=0))
        say(f"## {title}")
        for name, st in stats.items():
            say(bl.timed(name, st, 86))
        say(f"visits on the reported path of clip 0: {visits[0]} with nothing repeatable, {visits[1]} with the chorus repeatable, {visits[2]} with "
            f"chorus .. verse repeatable and the verse optional ({L} labels on the sheet); nothing-given outputs equal "
            f"la_viterbi_lattice_batch's bit for bit; every status LA_OK")
        m, base = stats[NEW[0]][0], stats[EXISTING[1]][0]
        say(f"{NEW[0]}: {m:.3f} beside {EXISTING[1]} {base:.3f} of the same build ({100 * (m / base - 1):+.1f} %)")
        for name in NEW[1:]:
            say(f"{name}: {stats[name][0]:.3f} ({100 * (stats[name][0] / base - 1):+.1f} % of {EXISTING[1]})")
        for name in EXISTING if parent is not None else ():
            say(bl.against_parent(name, stats[name], stats["parent commit: " + name]))
        say()
        del legs, outs, c
        torch.cuda.empty_cache()
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
