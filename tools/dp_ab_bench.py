"""A/B of the alignment DP entry points between two builds of the library in ONE process (profiles/lattice_refactor.txt).

    python tools/dp_ab_bench.py --parent-lib <liblyricalign_hip.so of a built checkout of the parent commit> [--runs 30] [--quick] [--out FILE]

la_viterbi_batch and la_viterbi_spans_batch (without spans, and with four optional lines) at 32 clips x 1500 frames x 26 labels --
tools/optional_spans_bench.py's three legs on its emissions -- and both entry points on one 5389-frame, 171-label song (8 waves,
backpointer masks in the workspace).  Both libraries are loaded with ctypes; per leg their outputs are compared bit for bit, then
the two are alternated call by call (caller-owned buffers, device events around one call, a synchronise after each).  The yardstick
is the parent: a leg passes when this build's median lies inside the parent's own min .. max of the same run.  --quick without
--parent-lib places this build's library against itself.
"""
from __future__ import annotations

import torch

import benchlib as bl

PRESENT = [True, True, False, True]
# (B, T, L, the lines that are optional in the third leg or None: emissions without a planted path, what the title says of the form)
SHAPES = [(32, 1500, 26, [6, 7, 6, 7], ""), (1, 5389, 171, None, " (8 waves, masks in the workspace)")]
QUICK = [(2, 160, 8, [2, 2, 2, 2], ""), (1, 400, 40, None, " (2 waves)")]


def leg_table(quick=False):
    """Per shape, the names the report gives the legs."""
    table = []
    for B, T, L, lines, form in QUICK if quick else SHAPES:
        at = f"{B} x {T} x {L}"
        table.append([f"la_viterbi_batch {at}{form}", f"la_viterbi_spans_batch, no spans, {at}"]
                     + ([f"la_viterbi_spans_batch, lines {'/'.join(map(str, lines))} optional, {at}"] if lines else []))
    return table


def main(argv=None):
    ap = bl.parser(parent_lib=True, quick=True)
    args = bl.parse(ap, argv)
    if not args.parent_lib and not args.quick:
        ap.error("--parent-lib is required (--quick alone places this build's library against itself)")
    report = bl.Report(args.out)
    say = report.say
    dev, lib = bl.open_gpu()
    from lyricalignment_amd.utils.alignment import spans_from_lines
    from lyricalignment_amd._lib import LIB_PATH
    libs = {"parent": bl.load_parent(args.parent_lib or LIB_PATH, ("viterbi", "viterbi_spans")), "new": lib}

    say(f"# alignment DP, parent commit's library against this one's on {torch.cuda.get_device_name(0)}: both loaded in one process, alternated call by call,")
    say(f"# median (min .. max) of {args.runs} calls after a warm-up of 3, device events around one call, ms.  Outputs compared bit for bit before timing.")
    all_ok = True
    for (B, T, L, lines, _), names in zip(QUICK if args.quick else SHAPES, leg_table(args.quick)):
        if lines:
            em = bl.planted(B, T, L, bl.sung_lines(lines, PRESENT), B + T + L, dev)
        else:
            em = (-torch.rand((B, T, L + 1), generator=torch.Generator().manual_seed(B + T + L)) * 12 - 1).to(dev)
        c = bl.case(em, *bl.sheet(B, T, L, dev))
        skips = [None, torch.full((B, L + 1), -1, dtype=torch.int32, device=dev)] + (
            [bl.rows(spans_from_lines(lines, [True] * len(lines)), B, dev)] if lines else [])
        for name, skip in zip(names, skips):
            legs = [(k, bl.dp_leg(libs[k], "viterbi" if skip is None else "viterbi_spans", c, skip)) for k in ("parent", "new")]
            bl.warm_up(legs)
            (fp, out_p), (fn, out_n) = legs[0][1], legs[1][1]
            same = bl.same_bits(out_p, out_n, bl.DP_OUT) and fp.workspace_bytes == fn.workspace_bytes
            assert bl.ok(out_n), "status not LA_OK"
            assert same, f"{name}: outputs differ between the two libraries"
            ts = bl.alternated(legs, args.runs, warmup=0)
            parent, new = bl.stat(ts["parent"]), bl.stat(ts["new"])
            all_ok &= bl.inside(new, parent)
            say(f"{name}")
            say(f"    parent {parent[0]:7.3f} ({parent[1]:.3f} .. {parent[2]:.3f})   new {new[0]:7.3f} ({new[1]:.3f} .. {new[2]:.3f})   outputs equal: {same}")
            say("    " + bl.against_parent("new median", new, parent))
    say(f"all new medians inside the parent's own min .. max: {all_ok}")
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
