"""Cost of the pronunciation alternatives (csrc/la_readings.hip: la_emissions_merge_readings in front of the lattice, la_reading_scores
behind it) beside the DP on the same lattice and beside a plain device copy of the same number of bytes.

    python tools/readings_bench.py [--runs 30] [--out profiles/readings.txt]

Two shapes on synthetic emissions -- 32 clips x 1500 frames x 26 labels and 1 song x 12000 frames x 800 labels -- with every fourth
position given two readings (the planted column's probability split between them); the emissions plant an even segmentation.
Legs, alternated call by call (caller-owned buffers, device events around one call, a synchronise after each):
  * la_emissions_merge_readings: expanded matrix -> folded matrix;
  * la_reading_scores on the DP's boundaries;
  * la_viterbi_batch on the folded matrix: the DP the two kernels sit around;
  * a device copy (hipMemcpyAsync through torch's copy_) of as many bytes as the fold reads plus writes, as one read and one write of half
    of them each: the memory system's rate for the same traffic.
The bar for the fold: (bytes of the expanded rows + bytes of the folded rows) at the copy's measured rate; the achieved fraction of it is
printed.  Every number is the median of `runs` calls after a warm-up; min .. max is printed next to it.  The fold is checked against a
float64 fold on the host (equal or adjacent float32) before anything is timed.
"""
from __future__ import annotations

import numpy as np
import torch

import benchlib as bl

SHAPES = [("32 clips x 1500 frames x 26 labels", 32, 1500, 26), ("1 song x 12000 frames x 800 labels", 1, 12000, 800)]


def main(argv=None):
    args = bl.parse(bl.parser(), argv)
    report = bl.Report(args.out)
    say = report.say
    dev, lib = bl.open_gpu()
    from lyricalignment_amd import _lib, ops
    from lyricalignment_amd._lib import ptr, stream_ptr
    from lyricalignment_amd.utils.alignment import _readings_of
    say(f"# pronunciation alternatives on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a warm-up of 3, "
        f"legs alternated call by call, device events around one call, ms; every fourth position has two readings")
    for title, B, T, L in SHAPES:
        em0 = bl.planted(B, T, L, list(range(L)), B + T + L, "cpu")
        labels = [list(range(1, L + 1)) for _ in range(B)]
        rd = _readings_of([[(n, [5000 + n]) for n in range(0, L, 4)] for _ in range(B)], labels)
        alt_h = rd.alt_start[0].tolist()
        X = rd.n_columns[0]
        em_x_h = torch.empty((B, T, X + 1))
        em_x_h[:, :, 0] = em0[:, :, 0]
        for n in range(L):
            if alt_h[n + 1] - alt_h[n] == 1:
                em_x_h[:, :, 1 + alt_h[n]] = em0[:, :, 1 + n]
            else:                                                          # the sheet's reading on even clips, the other one on odd clips
                w = torch.tensor([0.9, 0.1]).log()
                em_x_h[0::2, :, 1 + alt_h[n]: 1 + alt_h[n + 1]] = em0[0::2, :, 1 + n, None] + w
                em_x_h[1::2, :, 1 + alt_h[n]: 1 + alt_h[n + 1]] = em0[1::2, :, 1 + n, None] + w.flip(0)
        em_x, alt, ids = em_x_h.to(dev), rd.alt_start.to(dev), rd.lattice_ids.to(dev)
        n_lab = torch.full((B,), L, dtype=torch.int32, device=dev)
        nf = torch.full((B,), T, dtype=torch.int32, device=dev)
        em = torch.empty((B, T, L + 1), dtype=torch.float32, device=dev)
        reading = torch.empty((B, L), dtype=torch.int32, device=dev)
        col = torch.empty((B, X), dtype=torch.float64, device=dev)
        ops.merge_readings(em_x, alt, n_lab, nf, out=em)
        onset, offset, _, status = ops.viterbi_batch(em, ids, n_lab, nf)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        # the fold against float64 on the host (clip 0): equal or adjacent float32
        x64 = em_x_h[0].double().numpy()
        got = em[0].cpu().numpy()
        for n in range(L):
            grp = x64[:, 1 + alt_h[n]: 1 + alt_h[n + 1]]
            m = grp.max(axis=1)
            ref = (m + np.log(np.exp(grp - m[:, None]).sum(axis=1))).astype(np.float32) if grp.shape[1] > 1 else grp[:, 0].astype(np.float32)
            ok = (got[:, 1 + n] == ref) | (got[:, 1 + n] == np.nextafter(ref, np.float32(np.inf))) | (got[:, 1 + n] == np.nextafter(ref, np.float32(-np.inf)))
            assert ok.all(), f"fold of position {n} differs from the float64 fold"
        n_bytes = (em_x.numel() + em.numel()) * 4                          # one read of the expanded rows, one write of the folded rows
        src = torch.empty((n_bytes // 2,), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def merge():
            _lib.check(lib.la_emissions_merge_readings(ptr(em_x), em_x.stride(0), em_x.stride(1), ptr(alt), alt.stride(0), ptr(n_lab), ptr(nf),
                                                         B, T, L, X, ptr(em), em.stride(0), em.stride(1), stream_ptr()), "merge")

        def scores():
            _lib.check(lib.la_reading_scores(ptr(em_x), em_x.stride(0), em_x.stride(1), ptr(alt), alt.stride(0), ptr(n_lab), ptr(onset),
                                               ptr(offset), L, B, T, L, X, ptr(col), X, ptr(reading), L, stream_ptr()), "scores")

        legs = [("la_emissions_merge_readings", merge), ("la_reading_scores", scores),
                ("la_viterbi_batch on the folded matrix", lambda: ops.viterbi_batch(em, ids, n_lab, nf)),
                (f"device copy of {n_bytes // 2} bytes (read + write = the fold's traffic)", lambda: dst.copy_(src))]
        stats = bl.stats_of(bl.alternated(legs, args.runs))
        say(f"## {title}: {X} expanded columns, fold traffic {n_bytes / 1e6:.2f} MB")
        for name, st in stats.items():
            say(bl.timed(name, st, 76, 8, 4))
        med = [st[0] for st in stats.values()]
        rate = n_bytes / (med[3] * 1e-3) / 1e9
        say(f"copy rate {rate:.1f} GB/s; bar for the fold = its traffic at that rate = {med[3]:.4f} ms; achieved fraction {med[3] / med[0]:.2f} "
            f"(fold {n_bytes / (med[0] * 1e-3) / 1e9:.1f} GB/s); fold + scores = {100 * (med[0] + med[1]) / med[2]:.1f} % of the DP")
        picked = reading.cpu()
        say(f"readings picked: {int((picked[0] > 0).sum())} of {L} positions of clip 0 name the other reading"
            + (f", {int((picked[1] > 0).sum())} of clip 1" if B > 1 else ""))
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
