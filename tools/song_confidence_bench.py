"""Cost of the whole-song confidence for repeated lyric lines (la_alignment_posteriors_song; beyond 511 labels the REP face of
posterior_strip_kernel in csrc/la_posterior.hip) beside la_alignment_posteriors_lattice.

    python tools/song_confidence_bench.py [--runs 30] [--quick] [--out profiles/song_confidence.txt]

Two songs on synthetic emissions -- 12000 frames x 800 labels (R = 2 states per thread) and 12000 frames x 2500 labels (R = 8) -- in lines
of 10 labels; the emissions plant the sheet with its second line (the chorus) sung twice.  Legs, alternated call by call (caller-owned
buffers, device events around one call, a synchronise after each; no gamma output):
  * la_alignment_posteriors_lattice with nothing given, and with one onset anchor per line (+-1 s) plus every fourth line optional;
  * la_alignment_posteriors_song with nothing repeatable, on the same two lattices (outputs checked bit for bit against the lattice
    entry's);
  * la_alignment_posteriors_song with the chorus repeatable;
  * la_alignment_posteriors_song with the chorus repeatable, one anchor per line and every fourth line optional.
Every leg is asked about the onset / offset / path that la_viterbi_repeats_batch reports for its lattice.  The times are recorded, not
gated: there is nothing to derive a bound from.  Every number is the median of `runs` calls after a warm-up; min .. max is printed next to
it, and the ratios beside the lattice entry on the same lattice.
"""
from __future__ import annotations

import torch

import benchlib as bl

LEGS = ("la_alignment_posteriors_lattice, nothing given",
        "la_alignment_posteriors_song, nothing repeatable",
        "la_alignment_posteriors_song, one repeatable chorus",
        "la_alignment_posteriors_lattice, one anchor per line, every fourth line optional",
        "la_alignment_posteriors_song, nothing repeatable, one anchor per line, every fourth line optional",
        "la_alignment_posteriors_song, one repeatable chorus, one anchor per line, every fourth line optional")
SONGS = [("1 song x 12000 frames x 800 labels (R = 2)", 12000, 800), ("1 song x 12000 frames x 2500 labels (R = 8)", 12000, 2500)]
QUICK_SONGS = [("1 song x 4400 frames x 520 labels (R = 2)",) + bl.QUICK_STRIP[1:3]]
LINE, HOP, TOL_S = 10, 0.02, 1.0


def leg_table(quick=False):
    """Per shape, the names the report gives the legs."""
    return [list(LEGS) for _ in (QUICK_SONGS if quick else SONGS)]


def main(argv=None):
    args = bl.parse(bl.parser(quick=True), argv)
    report = bl.Report(args.out)
    say = report.say
    dev, lib = bl.open_gpu()
    from lyricalignment_amd import ops
    from lyricalignment_amd.utils.alignment import repeats_from_lines, spans_from_lines, windows_from_anchors
    B = 1

    say(f"# whole-song posteriors on the lattice with repeatable lines on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} "
        f"calls after a warm-up of 3, legs alternated call by call, device events around one call, ms")
    for title, T, L in QUICK_SONGS if args.quick else SONGS:
        lengths, starts = bl.lines_of(L, LINE)
        sung = bl.sung_lines(lengths, [2 if i == 1 else 1 for i in range(len(lengths))])
        c = bl.case(bl.planted(B, T, L, sung, T + L, dev), *bl.sheet(B, T, L, dev))
        sheet = bl.rows(spans_from_lines(lengths, [i % 4 == 3 for i in range(len(lengths))]), B, dev)
        chorus = bl.rows(repeats_from_lines(lengths, [i == 1 for i in range(len(lengths))]), B, dev)
        # one onset anchor per line where the planting begins the line's FIRST visit
        seg = T // (2 * len(sung) + 1)
        win = tuple(bl.rows(w, B, dev) for w in windows_from_anchors(L, T, onset_anchors=[(a, (2 * sung.index(a) + 1) * seg * HOP, TOL_S) for a in starts]))

        def leg(stem, skip=None, windows=None, repeat=None):
            """-> (call, outputs); every leg asks about its own lattice's DP result (a song leg: with its path)"""
            dp = ops.viterbi_repeats_batch(*c[3:], skip, 0.0, *(windows or (None, None)), repeat, 0.0)
            assert int(dp[3].abs().sum()) == 0
            return bl.posterior_leg(lib, stem, c, dp[:2], skip, windows, repeat, dp[4])

        legs = list(zip(LEGS, [leg("alignment_posteriors_lattice"), leg("alignment_posteriors_song"),
                               leg("alignment_posteriors_song", None, None, chorus), leg("alignment_posteriors_lattice", sheet, win),
                               leg("alignment_posteriors_song", sheet, win), leg("alignment_posteriors_song", sheet, win, chorus)]))
        bl.warm_up(legs)
        outs = [out for _, (_, out) in legs]
        for name, (_, out) in legs:
            assert bl.ok(out), f"{name}: status not LA_OK"
        assert bl.same_bits(outs[0], outs[1], bl.SPAN_OUT) and bl.same_bits(outs[3], outs[4], bl.SPAN_OUT), "nothing repeatable differs from the lattice entry"
        assert int(outs[1]["repeat_count"].abs().sum()) == 0 and int(outs[4]["repeat_count"].abs().sum()) == 0
        stats = bl.stats_of(bl.alternated(legs, args.runs, warmup=0))
        say(f"## {title}")
        for name, st in stats.items():
            say(bl.timed(name, st, 100, 9))
        for i in (2, 5):
            rc, vis = outs[i]["repeat_count"][0], outs[i]["present"][0]
            say(f"{LEGS[i]}: repeat_count of the chorus {float(rc[starts[1]]):.4f}, visits of its first label {float(vis[starts[1]]):.4f}, "
                f"of the label after it {float(vis[starts[2]]):.4f}")
        say("nothing-repeatable outputs equal la_alignment_posteriors_lattice's bit for bit on both lattices; every status LA_OK")
        for i, base in ((1, 0), (2, 0), (4, 3), (5, 3)):
            m, b0 = stats[LEGS[i]][0], stats[LEGS[base]][0]
            say(f"{LEGS[i]}: {m:.3f} beside {LEGS[base]} {b0:.3f} ({100 * (m / b0 - 1):+.1f} %)")
        say()
        del legs, outs, c
        torch.cuda.empty_cache()
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
