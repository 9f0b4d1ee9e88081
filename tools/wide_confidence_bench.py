"""Cost of the whole-song posteriors (la_alignment_posteriors_lattice beyond 511 labels: posterior_strip_kernel,
csrc/la_posterior.hip) beside the alignment DP on the same lattice (la_viterbi_lattice_batch).

    python tools/wide_confidence_bench.py [--runs 30] [--quick] [--parent-lib <liblyricalign_hip.so of the parent commit>] [--out profiles/wide_confidence.txt]

Two whole songs on synthetic emissions -- 12000 frames x 800 labels (2 states per thread) and 12000 frames x 2500 labels (8 states per
thread), both in lines of 10 labels; the emissions plant every line but each fourth.  Four lattices per song:
  * nothing given;
  * every window [0, T) and a null skip_from: what the window face costs when nothing is known;
  * one onset anchor per line (the line's first character within 1 s of where the unanchored DP put it);
  * anchors (around the sheet-only DP's result) plus every fourth line optional.
On each lattice two legs, alternated call by call (caller-owned buffers, device events around one call, a synchronise after each):
la_viterbi_lattice_batch, the yardstick, and la_alignment_posteriors_lattice on the DP's onset / offset (no gamma output).
With --parent-lib every posterior leg runs beside the parent commit's, alternated with it call by call: the four
la_alignment_posteriors_lattice legs of each song, and the lane-per-state sweeps at 32 clips x 1500 frames x 26 labels and 1 clip x 5389
frames x 200 labels (la_alignment_posteriors, la_alignment_posteriors_spans without a span, la_alignment_posteriors_windows with every
window open).  All seven outputs are checked bit for bit before anything is timed -- also on a song of 3000 frames x 1100 labels (4
states per thread), which is not timed -- and every leg's median is reported against the parent's min .. max of the same leg.
Every number is the median of `runs` calls after a warm-up; min .. max is printed next to it; every status is LA_OK before anything is timed.
"""
from __future__ import annotations

import torch

import benchlib as bl

LATTICES = ("nothing given", "all windows open", "one onset anchor per line, +-1 s", "anchors + every fourth line optional")
SONGS = [("1 song x 12000 frames x 800 labels (2 states per thread)", 12000, 800),
         ("1 song x 12000 frames x 2500 labels (8 states per thread)", 12000, 2500)]
QUICK_SONGS = [("1 song x 4400 frames x 520 labels (2 states per thread)",) + bl.QUICK_STRIP[1:3]]
BITS_ONLY = [("1 song x 3000 frames x 1100 labels (4 states per thread)", 3000, 1100)]
EXISTING = [("32 clips x 1500 frames x 26 labels (1 wave)", 32, 1500, 26), ("1 clip x 5389 frames x 200 labels (8 waves)", 1, 5389, 200)]
QUICK_EXISTING = [("2 clips x 160 frames x 8 labels (1 wave)",) + bl.QUICK_ONE_WAVE[:3], ("1 clip x 400 frames x 40 labels (2 waves)",) + bl.QUICK_MULTI_WAVE[:3]]
EXISTING_LEGS = (("la_alignment_posteriors", "alignment_posteriors"), ("la_alignment_posteriors_spans, no span", "alignment_posteriors_spans"),
                 ("la_alignment_posteriors_windows, all windows open", "alignment_posteriors_windows"))
LINE = 10
TOL_S = 1.0


def leg_table(quick=False):
    """Per shape, the names the report gives the legs."""
    return [[entry + ", " + name for name in LATTICES for entry in ("la_viterbi_lattice_batch", "la_alignment_posteriors_lattice")]
            for _ in (QUICK_SONGS if quick else SONGS)]


def main(argv=None):
    args = bl.parse(bl.parser(parent_lib=True, quick=True), argv)
    report = bl.Report(args.out)
    say = report.say
    dev, lib = bl.open_gpu()
    from lyricalignment_amd.utils.alignment import spans_from_lines
    parent = None
    if args.parent_lib:
        parent = bl.load_parent(args.parent_lib, ("viterbi", "alignment_posteriors", "alignment_posteriors_spans", "alignment_posteriors_windows",
                                                  "alignment_posteriors_lattice"))

    def measure(title, legs):
        """-> {name: (median, min, max)}; every status LA_OK before anything is timed"""
        bl.warm_up(legs)
        for name, (_, out) in legs:
            assert bl.ok(out), f"{name}: status not LA_OK"
        ts = bl.alternated(legs, args.runs, warmup=0)
        say(f"## {title}")
        return bl.stats_of(ts)

    say(f"# whole-song posteriors on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a warm-up of 3, "
        f"legs alternated call by call, device events around one call, ms")
    for title, T, L in (QUICK_SONGS if args.quick else SONGS) + (BITS_ONLY if parent is not None and not args.quick else []):
        lengths, starts = bl.lines_of(L, LINE)
        optional = [i % 4 == 3 for i in range(len(lengths))]
        c = bl.case(bl.planted(1, T, L, bl.sung_lines(lengths, [not o for o in optional]), T + L, dev), *bl.sheet(1, T, L, dev))
        skip = bl.rows(spans_from_lines(lengths, optional), 1, dev)

        plain, sheet_only = bl.dp_leg(lib, "viterbi", c), bl.dp_leg(lib, "viterbi_lattice", c, skip)
        bl.warm_up([("", plain), ("", sheet_only)], 1)
        assert bl.ok(plain[1]) and bl.ok(sheet_only[1])
        lattices = [(None, None), (None, bl.open_windows(1, T, L, dev)), (None, bl.anchored_windows(plain[1]["onset"], starts, T, L, TOL_S)),
                    (skip, bl.anchored_windows(sheet_only[1]["onset"], starts, T, L, TOL_S))]
        legs, beside = [], []
        for name, (sk, win) in zip(LATTICES, lattices):
            dp = bl.dp_leg(lib, "viterbi_lattice", c, sk, win)
            bl.warm_up([("", dp)], 1)
            frames = (dp[1]["onset"], dp[1]["offset"])
            post = bl.posterior_leg(lib, "alignment_posteriors_lattice", c, frames, sk, win)
            legs += [("la_viterbi_lattice_batch, " + name, dp), ("la_alignment_posteriors_lattice, " + name, post)]
            ws_mb = post[0].workspace_bytes / 1e6
            if parent is not None:
                theirs = bl.posterior_leg(parent, "alignment_posteriors_lattice", c, frames, sk, win)
                bl.warm_up([("", post), ("", theirs)], 1)
                assert bl.ok(post[1]) and bl.same_bits(post[1], theirs[1], bl.SPAN_OUT), f"{title}, {name}: outputs differ from the parent commit's"
                beside.append(("parent commit: la_alignment_posteriors_lattice, " + name, theirs))
        if (title, T, L) in BITS_ONLY:
            say(f"## {title}: la_alignment_posteriors_lattice on the four lattices, all seven outputs equal the parent commit's bit for bit (not timed)")
            continue
        stats = measure(title, legs + beside)
        for (dn, _), (pn, _) in zip(legs[0::2], legs[1::2]):
            say(bl.timed(dn, stats[dn], 72, 9))
            say(bl.timed(pn, stats[pn], 72, 9) + f"   {stats[pn][0] / stats[dn][0]:5.2f} x the DP on the same lattice")
        open_same = bl.same_bits(legs[1][1][1], legs[3][1][1], bl.SPAN_OUT)
        last = legs[-1][1][1]
        say(f"workspace {ws_mb:.0f} MB; every status LA_OK; all-open outputs equal the nothing-given ones bit for bit: {open_same}; with the sheet "
            f"{int((last['present'][0] < 0.5).sum())} of {L} labels have sung_prob < 0.5, log_z {float(last['log_z'][0]):.3f}")
        for name, _ in legs[1::2] if parent is not None else []:
            say(bl.against_parent(name, stats[name], stats["parent commit: " + name]) + "; outputs bit-equal")
        del c, legs, beside, plain, sheet_only, lattices
        torch.cuda.empty_cache()

    for title, B, T, L in (QUICK_EXISTING if args.quick else EXISTING) if parent is not None else ():
        c = bl.case(bl.planted(B, T, L, list(range(L)), B + T + L, dev), *bl.sheet(B, T, L, dev))
        none = torch.full((B, L + 1), -1, dtype=torch.int32, device=dev)
        dp = bl.dp_leg(lib, "viterbi", c)
        bl.warm_up([("", dp)], 1)
        frames = (dp[1]["onset"], dp[1]["offset"])
        legs = []
        for who, lib_ in (("", lib), ("parent commit: ", parent)):
            for (name, stem), (sk, win) in zip(EXISTING_LEGS, ((None, None), (none, None), (None, bl.open_windows(B, T, L, dev)))):
                legs.append((who + name, bl.posterior_leg(lib_, stem, c, frames, sk, win)))
        bl.warm_up(legs, 1)
        for i in range(3):                                    # the plain entry writes no span outputs
            assert bl.same_bits(legs[i][1][1], legs[3 + i][1][1], bl.SPAN_OUT if i else bl.POSTERIOR_OUT), f"{legs[i][0]}: outputs differ from the parent commit's"
        stats = measure(title + ": the existing entries beside the parent's", legs)
        for name, st in stats.items():
            say(bl.timed(name, st, 72, 9))
        for name, _ in EXISTING_LEGS:
            say(bl.against_parent(name, stats[name], stats["parent commit: " + name]) + "; outputs bit-equal")
        del c, legs
        torch.cuda.empty_cache()
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
