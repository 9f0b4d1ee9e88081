"""Cost of the alignment DP with per-state frame windows (la_viterbi_windows_batch) beside la_viterbi_batch and
la_viterbi_spans_batch; all three are instantiations of one kernel in csrc/la_viterbi.hip.

    python tools/anchored_bench.py [--runs 30] [--parent-lib <liblyricalign_hip.so of the parent commit>] [--out profiles/anchored_alignment.txt]

Two shapes on synthetic emissions -- 32 clips x 1500 frames x 26 labels (four lines of 6 / 7 / 6 / 7 characters; one wave, masks in LDS)
and one song of 5389 frames x 200 labels (four lines of 50; 8 waves, masks in the workspace); the emissions plant lines 1, 2 and 4.
Legs, alternated call by call (caller-owned buffers, device events around one call, a synchronise after each):
  * la_viterbi_batch;
  * la_viterbi_spans_batch without a span, and with the four lines optional;
  * la_viterbi_windows_batch with every window [0, T) and a null skip_from: what the window instantiation costs when nothing is known;
  * la_viterbi_windows_batch with one onset anchor per line (the line's first character within 1 s of where the unanchored DP put it);
  * la_viterbi_windows_batch with those anchors and the four lines optional.
With --parent-lib the parent commit's la_viterbi_batch and span-free la_viterbi_spans_batch run in the same alternation: the yardstick of
the all-open leg is the parent's span-free la_viterbi_spans_batch (inside its min .. max or not).
Every number is the median of `runs` calls after a warm-up; min .. max is printed next to it.  The all-open outputs are checked bit for
bit against la_viterbi_batch's, and every anchored leg's status is LA_OK, before anything is timed.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PRESENT = [True, True, False, True]
SHAPES = [("32 clips x 1500 frames x 26 labels (1 wave, masks in LDS)", 32, 1500, [6, 7, 6, 7]),
          ("1 song x 5389 frames x 200 labels (8 waves, masks in the workspace)", 1, 5389, [50, 50, 50, 50])]
TOL_S = 1.0


def _time_once(torch, fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    sys.path.insert(0, os.path.join(HERE, ".."))
    import torch
    from lyricalignment_amd import _lib
    from lyricalignment_amd._lib import SYMBOLS, lib, ptr, stream_ptr
    from lyricalignment_amd.utils.alignment import spans_from_lines, windows_from_anchors
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("la_viterbi_workspace_bytes", "la_viterbi_batch", "la_viterbi_spans_workspace_bytes", "la_viterbi_spans_batch"):
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = SYMBOLS[name]

    say(f"# alignment DP with per-state frame windows on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a "
        f"warm-up of 3, legs alternated call by call, device events around one call, ms")
    for title, B, T, line_lengths in SHAPES:
        L = sum(line_lengths)
        # emissions -rand * 12 - 1 with a 0.8 * 12 bonus on an even segmentation of the SUNG labels (lines 1, 2 and 4)
        g = torch.Generator().manual_seed(B + T + L)
        em = -torch.rand((B, T, L + 1), generator=g) * 12 - 1
        sung, pos = [], 0
        for n_chars, here in zip(line_lengths, PRESENT):
            sung += list(range(pos, pos + n_chars)) if here else []
            pos += n_chars
        seg = T // (2 * len(sung) + 1)
        for i, n in enumerate(sung):
            em[:, (2 * i + 1) * seg:(2 * i + 2) * seg, 1 + n] += 9.6
        for i in range(len(sung) + 1):
            em[:, 2 * i * seg:(2 * i + 1) * seg, 0] += 9.6
        em = em.to(dev)
        labels = torch.arange(1, L + 1, dtype=torch.int32).repeat(B, 1).to(dev)
        n_labels = torch.full((B,), L, dtype=torch.int32, device=dev)
        n_frames = torch.full((B,), T, dtype=torch.int32, device=dev)
        skip_none = torch.full((B, L + 1), -1, dtype=torch.int32, device=dev)
        skip_all = torch.tensor(spans_from_lines(line_lengths, [True] * len(line_lengths)), dtype=torch.int32).repeat(B, 1).to(dev)
        starts = [sum(line_lengths[:i]) for i in range(len(line_lengths))]

        def outputs():
            return (torch.full((B, L), -7, dtype=torch.int32, device=dev), torch.full((B, L), -7, dtype=torch.int32, device=dev),
                    torch.full((B,), -7.0, dtype=torch.float64, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev))

        def workspace(L_, query):
            need = ctypes.c_size_t(0)
            assert getattr(L_, query)(B, T, L, ctypes.byref(need)) == 0
            return torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev), need.value

        def plain_leg(L_):
            out, (ws, need) = outputs(), workspace(L_, "la_viterbi_workspace_bytes")

            def fn():
                on, off, score, status = out
                assert L_.la_viterbi_batch(ptr(em), em.stride(0), em.stride(1), ptr(labels), L, ptr(n_labels), ptr(n_frames), B, T, L, ptr(on),
                                           ptr(off), L, ptr(score), ptr(status), ptr(ws), need, stream_ptr()) == 0
            return fn, out

        def spans_leg(L_, skip):
            out, (ws, need) = outputs(), workspace(L_, "la_viterbi_spans_workspace_bytes")

            def fn():
                on, off, score, status = out
                assert L_.la_viterbi_spans_batch(ptr(em), em.stride(0), em.stride(1), ptr(labels), L, ptr(n_labels), ptr(n_frames), B, T, L, ptr(on),
                                                 ptr(off), L, ptr(score), ptr(status), ptr(skip), L + 1, 0.0, ptr(ws), need, stream_ptr()) == 0
            return fn, out

        def windows_leg(skip, lo, hi):
            out, (ws, need) = outputs(), workspace(lib(), "la_viterbi_windows_workspace_bytes")

            def fn():
                on, off, score, status = out
                assert lib().la_viterbi_windows_batch(ptr(em), em.stride(0), em.stride(1), ptr(labels), L, ptr(n_labels), ptr(n_frames), B, T, L,
                                                      ptr(on), ptr(off), L, ptr(score), ptr(status), ptr(skip), L + 1 if skip is not None else 0, 0.0,
                                                      ptr(lo), ptr(hi), 2 * L + 1, ptr(ws), need, stream_ptr()) == 0, _lib.last_error()
            return fn, out

        def anchored(onsets):
            """Windows of every clip from one onset anchor per line, at the frame the given result has for the line's first sung character
            (a line that was left out: the next line's)."""
            lo_rows, hi_rows = [], []
            for b in range(B):
                anchors, nxt = [], None
                for a in reversed(starts):
                    f = int(onsets[b, a])
                    nxt = f if f >= 0 else nxt
                    anchors.append((a, (nxt if nxt is not None else T - 1) * 0.02, TOL_S))
                lo, hi = windows_from_anchors(L, T, onset_anchors=anchors)
                lo_rows.append(lo); hi_rows.append(hi)
            return torch.tensor(lo_rows, dtype=torch.int32).to(dev), torch.tensor(hi_rows, dtype=torch.int32).to(dev)

        legs = [("la_viterbi_batch", plain_leg(lib())), ("la_viterbi_spans_batch, no span", spans_leg(lib(), skip_none)),
                ("la_viterbi_spans_batch, four optional lines", spans_leg(lib(), skip_all))]
        for _, (fn, _) in legs:
            fn()
        torch.cuda.synchronize()
        open_lo = torch.zeros((B, 2 * L + 1), dtype=torch.int32, device=dev)
        open_hi = torch.full((B, 2 * L + 1), T, dtype=torch.int32, device=dev)
        lo_a, hi_a = anchored(legs[0][1][1][0].cpu())
        lo_s, hi_s = anchored(legs[2][1][1][0].cpu())
        legs += [("la_viterbi_windows_batch, all windows open", windows_leg(None, open_lo, open_hi)),
                 ("la_viterbi_windows_batch, one onset anchor per line, +-1 s", windows_leg(None, lo_a, hi_a)),
                 ("la_viterbi_windows_batch, anchors + four optional lines", windows_leg(skip_all, lo_s, hi_s))]
        if parent is not None:
            legs += [("parent commit: la_viterbi_batch", plain_leg(parent)), ("parent commit: la_viterbi_spans_batch, no span", spans_leg(parent, skip_none))]
        for _ in range(3):
            for _, (fn, _) in legs:
                fn()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(legs[0][1][1], legs[3][1][1])), "all-open outputs differ from la_viterbi_batch"
        assert all(torch.equal(a, b) for a, b in zip(legs[0][1][1], legs[1][1][1])), "span-free outputs differ from la_viterbi_batch"
        for name, (_, out) in legs:
            assert int(out[3].abs().sum()) == 0, f"{name}: status not LA_OK"
        same = all(torch.equal(a, b) for a, b in zip(legs[2][1][1], legs[5][1][1]))      # anchors laid around the span DP's own result
        closed = float(((lo_a > 0) | (hi_a < T)).float().mean())
        ts = [[] for _ in legs]
        for _ in range(args.runs):
            for i, (_, (fn, _)) in enumerate(legs):
                ts[i].append(_time_once(torch, fn))
        say(f"## {title}")
        base = statistics.median(ts[0])
        stats = []
        for (name, _), t in zip(legs, ts):
            m, lo_t, hi_t = statistics.median(t), min(t), max(t)
            stats.append((m, lo_t, hi_t))
            say(f"{name:62s} {m:8.3f} ({lo_t:.3f} .. {hi_t:.3f})   {m / base:5.2f} x la_viterbi_batch")
        say(f"all-open outputs equal la_viterbi_batch's bit for bit; anchors narrow {100 * closed:.0f} % of the states' windows; every status LA_OK; "
            f"anchored + optional result equals the unanchored one: {same}")
        if parent is not None:
            m, (pm, plo, phi) = stats[3][0], stats[-1]
            where = "inside" if plo <= m <= phi else ("BELOW" if m < plo else "ABOVE")
            say(f"all windows open {m:.3f} against the parent's span-free la_viterbi_spans_batch {pm:.3f} ({plo:.3f} .. {phi:.3f}): {where} its "
                f"min .. max ({100 * (m / pm - 1):+.1f} % of its median)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
