"""Cost of the confidences on the lattice with per-state frame windows (la_alignment_posteriors_windows) beside la_alignment_posteriors and
la_alignment_posteriors_spans; all three are instantiations of one kernel in csrc/la_posterior.hip.

    python tools/anchored_confidence_bench.py [--runs 30] [--parent-lib <liblyricalign_hip.so of the parent commit>] [--out profiles/anchored_confidence.txt]

Two shapes on the synthetic emissions of tools/anchored_bench.py -- 32 clips x 1500 frames x 26 labels (four lines of 6 / 7 / 6 / 7 characters;
one wave) and one song of 5389 frames x 200 labels (four lines of 50; 8 waves); the emissions plant lines 1, 2 and 4.
Legs, alternated call by call (caller-owned buffers, no gamma output, boundary_window 2, device events around one call, a synchronise after each):
  * la_alignment_posteriors;
  * la_alignment_posteriors_spans without a span, and with the four lines optional;
  * la_alignment_posteriors_windows with every window [0, T) and a null skip_from: what the window instantiation costs when nothing is known;
  * la_alignment_posteriors_windows with one onset anchor per line (the line's first character within 1 s of where the unanchored DP put it);
  * la_alignment_posteriors_windows with those anchors and the four lines optional.
The DP that supplies each leg's onset / offset runs once, untimed.  With --parent-lib the parent commit's la_alignment_posteriors and
la_alignment_posteriors_spans (no span, four lines) run in the same alternation: each existing entry of this tree is placed against the
parent's own min .. max, and the all-open leg against the span-free la_alignment_posteriors_spans on the same inputs.
Every number is the median of `runs` calls after a warm-up; min .. max is printed next to it.  Before anything is timed the all-open outputs
are checked bit for bit against la_alignment_posteriors_spans', and every leg's status is LA_OK.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PRESENT = [True, True, False, True]
SHAPES = [("32 clips x 1500 frames x 26 labels (1 wave)", 32, 1500, [6, 7, 6, 7]),
          ("1 song x 5389 frames x 200 labels (8 waves)", 1, 5389, [50, 50, 50, 50])]
TOL_S = 1.0
DP_GATE_PERCENT = 5.7      # what the window gate cost the DP at 32 x 1500 x 26 (profiles/anchored_alignment.txt)


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
    from lyricalignment_amd import _lib, ops
    from lyricalignment_amd._lib import SYMBOLS, lib, ptr, stream_ptr
    from lyricalignment_amd.utils.alignment import spans_from_lines, windows_from_anchors
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("la_alignment_posteriors_workspace_bytes", "la_alignment_posteriors", "la_alignment_posteriors_spans_workspace_bytes",
                     "la_alignment_posteriors_spans"):
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = SYMBOLS[name]

    say(f"# confidences on the lattice with per-state frame windows on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls "
        f"after a warm-up of 3, legs alternated call by call, device events around one call, ms; boundary_window 2, no gamma output")
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

        # the DPs that supply onset / offset, once, untimed
        dp_plain = ops.viterbi_batch(em, labels, n_labels, n_frames)
        dp_spans = ops.viterbi_spans_batch(em, labels, n_labels, n_frames, skip_all, 0.0)
        open_lo = torch.zeros((B, 2 * L + 1), dtype=torch.int32, device=dev)
        open_hi = torch.full((B, 2 * L + 1), T, dtype=torch.int32, device=dev)
        lo_a, hi_a = anchored(dp_plain[0].cpu())
        lo_s, hi_s = anchored(dp_spans[0].cpu())
        dp_anch = ops.viterbi_windows_batch(em, labels, n_labels, n_frames, lo_a, hi_a)
        dp_anch_s = ops.viterbi_windows_batch(em, labels, n_labels, n_frames, lo_s, hi_s, skip_all, 0.0)
        torch.cuda.synchronize()
        for dp in (dp_plain, dp_spans, dp_anch, dp_anch_s):
            assert int(dp[3].abs().sum()) == 0, "a DP leg is not LA_OK"

        def outputs(n):
            out = [torch.full((B, L), -7.0, dtype=torch.float32, device=dev) for _ in range(3)] + [
                torch.full((B,), -7.0, dtype=torch.float64, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev)]
            if n == 7:
                out += [torch.full((B, L), -7.0, dtype=torch.float32, device=dev), torch.full((B, L + 1), -7.0, dtype=torch.float32, device=dev)]
            return out

        def workspace(L_, query):
            need = ctypes.c_size_t(0)
            assert getattr(L_, query)(B, T, L, ctypes.byref(need)) == 0
            return torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev), need.value

        def plain_leg(L_):
            out, (ws, need) = outputs(5), workspace(L_, "la_alignment_posteriors_workspace_bytes")
            on, off = dp_plain[0], dp_plain[1]

            def fn():
                occ, onp, offp, log_z, status = out
                assert L_.la_alignment_posteriors(ptr(em), em.stride(0), em.stride(1), ptr(labels), L, ptr(n_labels), ptr(n_frames), B, T, L,
                                                  ptr(on), ptr(off), L, 2, ptr(occ), ptr(onp), ptr(offp), ptr(log_z), ptr(status), 0, 0, 0,
                                                  ptr(ws), need, stream_ptr()) == 0
            return fn, out

        def spans_leg(L_, skip, dp):
            out, (ws, need) = outputs(7), workspace(L_, "la_alignment_posteriors_spans_workspace_bytes")
            on, off = dp[0], dp[1]

            def fn():
                occ, onp, offp, log_z, status, pres, skp = out
                assert L_.la_alignment_posteriors_spans(ptr(em), em.stride(0), em.stride(1), ptr(labels), L, ptr(n_labels), ptr(n_frames), B, T, L,
                                                        ptr(on), ptr(off), L, 2, ptr(skip), L + 1, 0.0, ptr(occ), ptr(onp), ptr(offp), ptr(pres),
                                                        ptr(skp), ptr(log_z), ptr(status), 0, 0, 0, ptr(ws), need, stream_ptr()) == 0
            return fn, out

        def windows_leg(skip, lo, hi, dp):
            out, (ws, need) = outputs(7), workspace(lib(), "la_alignment_posteriors_windows_workspace_bytes")
            on, off = dp[0], dp[1]

            def fn():
                occ, onp, offp, log_z, status, pres, skp = out
                assert lib().la_alignment_posteriors_windows(ptr(em), em.stride(0), em.stride(1), ptr(labels), L, ptr(n_labels), ptr(n_frames), B, T,
                                                             L, ptr(on), ptr(off), L, 2, ptr(skip), L + 1, 0.0, ptr(lo), ptr(hi), 2 * L + 1, ptr(occ),
                                                             ptr(onp), ptr(offp), ptr(pres), ptr(skp), ptr(log_z), ptr(status), 0, 0, 0, ptr(ws),
                                                             need, stream_ptr()) == 0, _lib.last_error()
            return fn, out

        legs = [("la_alignment_posteriors", plain_leg(lib())),
                ("la_alignment_posteriors_spans, no span", spans_leg(lib(), skip_none, dp_plain)),
                ("la_alignment_posteriors_spans, four optional lines", spans_leg(lib(), skip_all, dp_spans)),
                ("la_alignment_posteriors_windows, all windows open", windows_leg(None, open_lo, open_hi, dp_plain)),
                ("la_alignment_posteriors_windows, one onset anchor per line, +-1 s", windows_leg(None, lo_a, hi_a, dp_anch)),
                ("la_alignment_posteriors_windows, anchors + four optional lines", windows_leg(skip_all, lo_s, hi_s, dp_anch_s))]
        if parent is not None:
            legs += [("parent commit: la_alignment_posteriors", plain_leg(parent)),
                     ("parent commit: la_alignment_posteriors_spans, no span", spans_leg(parent, skip_none, dp_plain)),
                     ("parent commit: la_alignment_posteriors_spans, four optional lines", spans_leg(parent, skip_all, dp_spans))]
        for _ in range(3):
            for _, (fn, _) in legs:
                fn()
        torch.cuda.synchronize()
        assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(legs[1][1][1], legs[3][1][1])), \
            "all-open outputs differ from la_alignment_posteriors_spans'"
        assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(legs[0][1][1], legs[1][1][1][:5])), \
            "span-free outputs differ from la_alignment_posteriors'"
        for name, (_, out) in legs:
            assert int(out[4].abs().sum()) == 0, f"{name}: status not LA_OK"
        closed = float(((lo_a > 0) | (hi_a < T)).float().mean())
        wlp_a = (legs[4][1][1][3] - legs[0][1][1][3]).cpu()
        wlp_s = (legs[5][1][1][3] - legs[2][1][1][3]).cpu()
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
            say(f"{name:70s} {m:8.3f} ({lo_t:.3f} .. {hi_t:.3f})   {m / base:5.2f} x la_alignment_posteriors")
        say(f"all-open outputs equal la_alignment_posteriors_spans' bit for bit; anchors narrow {100 * closed:.0f} % of the states' windows; every "
            f"status LA_OK; window_log_prob (windowed log_z - free log_z) of the anchored legs: {float(wlp_a.min()):.3f} .. {float(wlp_a.max()):.3f} "
            f"(anchors), {float(wlp_s.min()):.3f} .. {float(wlp_s.max()):.3f} (anchors + optional lines)")
        for i, j, what in ((3, 1, "all windows open against la_alignment_posteriors_spans, no span"),
                           (4, 1, "one onset anchor per line against la_alignment_posteriors_spans, no span"),
                           (5, 2, "anchors + four optional lines against la_alignment_posteriors_spans, four optional lines")):
            say(f"{what}: {stats[i][0]:.3f} against {stats[j][0]:.3f} ({100 * (stats[i][0] / stats[j][0] - 1):+.1f} %; the DP's gate measured "
                f"+{DP_GATE_PERCENT} % all open)")
        if parent is not None:
            for i in range(3):
                m, (pm, plo, phi) = stats[i][0], stats[6 + i]
                where = "inside" if plo <= m <= phi else ("BELOW" if m < plo else "ABOVE")
                say(f"{legs[i][0]}: {m:.3f} against the parent's {pm:.3f} ({plo:.3f} .. {phi:.3f}): {where} its min .. max "
                    f"({100 * (m / pm - 1):+.1f} % of its median)")
        say("")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
