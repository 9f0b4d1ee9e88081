"""Cost of the off-sheet slots (csrc/la_offsheet.hip: la_emissions_offsheet_columns in front of the lattice) beside the DP with and
without the slots, and the two store mappings of the kernel beside each other.

    python tools/offsheet_bench.py [--runs 30] [--out profiles/offsheet.txt]

Two shapes on synthetic emissions -- 32 clips x 1500 frames x 26 labels plus 3 slots, and 1 song x 12000 frames x 800 labels plus 61
slots -- with a slot before every line (and one after the last); the emissions plant an even segmentation in which every slot is sung.
Legs, alternated call by call (device events around one call, a synchronise after each):
  * la_emissions_offsheet_columns, slot-major (a row's value staged in LDS, lanes on (row, slot) pairs): the form the library has;
  * with the experiment build only (bash tools/build_variant.sh lab -DLA_EXPERIMENTS, LA_LIB_PATH=ab/lab/liblyricalign_hip.so): the same
    entry frame-major (its developer switch LA_OFFSHEET_FORM=rows: a lane owns a frame and walks the slots), checked for the same bits;
  * the DP on the sheet without slots (ops.viterbi_batch on L labels);
  * the DP on the sheet with slots (L' = L + F labels, every slot a one-label optional span: ops.viterbi_spans_batch up to 511 labels,
    ops.viterbi_lattice_batch beyond).
Every number is the median of `runs` calls after a warm-up; min .. max is printed next to it.  Before anything is timed the kernel is
checked against the float64 formula on the host (equal or adjacent float32; the share of exactly equal values is printed).  No existing kernel is compiled differently by this addition, so there is no A/B of the existing entries.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

import benchlib as bl

SHAPES = [("32 clips x 1500 frames x 26 labels + 3 slots", 32, 1500, 26, 2), ("1 song x 12000 frames x 800 labels + 61 slots", 1, 12000, 800, 60)]      # (.., lines)
PENALTY = math.log(100.0)


def main(argv=None):
    args = bl.parse(bl.parser(), argv)
    report = bl.Report(args.out)
    say = report.say
    dev, lib = bl.open_gpu()
    from lyricalignment_amd import _lib, ops
    from lyricalignment_amd._lib import ptr, stream_ptr
    from lyricalignment_amd.utils.alignment import POSTERIOR_MAX_LABELS, _off_sheet_of, _skip_from_of_spans
    say(f"# off-sheet slots on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a warm-up of 3, legs alternated "
        f"call by call, device events around one call, ms; penalty ln 100")
    say("# no existing kernel is compiled differently by this addition: no A/B of the existing entries")
    for title, B, T, L, n_lines in SHAPES:
        starts = [i * L // n_lines for i in range(n_lines)]
        off = _off_sheet_of("bench", [starts + [L]] * B, PENALTY, [list(range(1, L + 1))] * B)
        F, Lx = len(starts) + 1, L + len(starts) + 1
        plain = bl.case(bl.planted(B, T, L, list(range(L)), B + T + L, dev), *bl.sheet(B, T, L, dev))
        em = bl.planted(B, T, Lx, list(range(Lx)), B + T + Lx, dev)
        em[:, :, 0].clamp_(max=-1e-6)                                  # log-probabilities: silence below 0
        cols, n_slots = off.slot_cols.to(dev), off.n_slots.to(dev)
        em[:, :, 1 + cols[0].long()] = -1000.0                         # what the head and the prep leave at a slot
        ids = off.lattice_ids.to(dev)
        n_lab = torch.full((B,), Lx, dtype=torch.int32, device=dev)
        nf = torch.full((B,), T, dtype=torch.int32, device=dev)
        skip = _skip_from_of_spans(off.optional_spans, off.label_lists).to(dev)

        def kernel(form):
            def call():
                if form:
                    os.environ["LA_OFFSHEET_FORM"] = form
                _lib.check(lib.la_emissions_offsheet_columns(ptr(em), em.stride(0), em.stride(1), ptr(cols), cols.stride(0), ptr(n_slots), ptr(nf),
                                                               B, T, Lx, F, PENALTY, stream_ptr()), "offsheet")
                os.environ.pop("LA_OFFSHEET_FORM", None)
            return call

        # against the float64 formula (clip 0); the experiment build's other form against this one
        both = _lib.has_experiments()
        if both:
            kernel("rows")()
            by_rows = em.clone()
            em[:, :, 1 + cols[0].long()] = -1000.0
        kernel("")()
        torch.cuda.synchronize()
        assert not both or by_rows.cpu().numpy().tobytes() == em.cpu().numpy().tobytes(), "the two forms differ"
        host = em[0].cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.log(-np.expm1(host[:, 0].astype(np.float64))) - PENALTY
        ref = np.where(v > -1000.0, v, -1000.0).astype(np.float32)
        got = host[:, 1 + off.slot_cols[0].long().numpy()]
        near = (got == ref[:, None]) | (np.nextafter(got, ref[:, None]) == ref[:, None])
        assert near.all(), "the kernel differs from the float64 formula by more than one float32 step"
        dp_with = "viterbi_spans_batch" if Lx <= POSTERIOR_MAX_LABELS else "viterbi_lattice_batch"
        st = ops.viterbi_batch(plain.em, plain.labels, plain.n_labels, plain.n_frames)[3], getattr(ops, dp_with)(em, ids, n_lab, nf, skip, 0.0)[3]
        torch.cuda.synchronize()
        assert all(int(s.abs().sum()) == 0 for s in st)
        used = int((getattr(ops, dp_with)(em, ids, n_lab, nf, skip, 0.0)[0][0, cols[0].long()] >= 0).sum())
        legs = [("la_emissions_offsheet_columns, slot-major", kernel(""))]
        legs += [("la_emissions_offsheet_columns, frame-major (LA_OFFSHEET_FORM=rows)", kernel("rows"))] if both else []
        legs += [(f"ops.viterbi_batch, {L} labels, no slots", lambda: ops.viterbi_batch(plain.em, plain.labels, plain.n_labels, plain.n_frames)),
                (f"ops.{dp_with}, {Lx} labels, {F} slots", lambda: getattr(ops, dp_with)(em, ids, n_lab, nf, skip, 0.0))]
        stats = bl.stats_of(bl.alternated(legs, args.runs))
        say(f"## {title}: {B * T * F} scattered 4-byte stores, {B * T} float64 log / expm1 pairs; {used} of {F} slots of clip 0 used by the DP")
        for name, s in stats.items():
            say(bl.timed(name, s, 64, 8, 4))
        med = [s[0] for s in stats.values()]
        med = med if both else [med[0], float("nan")] + med[1:]
        forms = f"slot-major / frame-major = {med[0] / med[1]:.2f}; " if both else ""
        say(f"exactly equal to the float64 formula: {float((got == ref[:, None]).mean()):.6f} of {got.size} values of clip 0 (the rest one float32 step "
            f"away); {forms}kernel = {100 * med[0] / med[3]:.2f} % of the DP with slots; "
            f"DP with slots / without = {med[3] / med[2]:.2f}")
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
