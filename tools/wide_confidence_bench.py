"""Cost of the whole-song posteriors (la_alignment_posteriors_lattice beyond 511 labels: posterior_strip_kernel,
csrc/la_posterior.hip) beside the alignment DP on the same lattice (la_viterbi_lattice_batch).

    python tools/wide_confidence_bench.py [--runs 30] [--parent-lib <liblyricalign_hip.so of the parent commit>] [--out profiles/wide_confidence.txt]

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

import argparse
import ctypes
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LATTICES = ("nothing given", "all windows open", "one onset anchor per line, +-1 s", "anchors + every fourth line optional")
SONGS = [("1 song x 12000 frames x 800 labels (2 states per thread)", 12000, 800),
         ("1 song x 12000 frames x 2500 labels (8 states per thread)", 12000, 2500)]
BITS_ONLY = [("1 song x 3000 frames x 1100 labels (4 states per thread)", 3000, 1100)]
EXISTING = [("32 clips x 1500 frames x 26 labels (1 wave)", 32, 1500, 26), ("1 clip x 5389 frames x 200 labels (8 waves)", 1, 5389, 200)]
LINE = 10
TOL_S = 1.0
HOP = 0.02


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
        for stem in ("viterbi", "alignment_posteriors", "alignment_posteriors_spans", "alignment_posteriors_windows", "alignment_posteriors_lattice"):
            for name in (f"la_{stem}_workspace_bytes", f"la_{stem}_batch" if stem == "viterbi" else f"la_{stem}"):
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = SYMBOLS[name]

    def planted(B, T, L, sung, seed):
        """emissions -rand * 12 - 1 with a 0.8 * 12 bonus on an even segmentation of the SUNG labels"""
        g = torch.Generator().manual_seed(seed)
        em = -torch.rand((B, T, L + 1), generator=g) * 12 - 1
        seg = T // (2 * len(sung) + 1)
        for i, n in enumerate(sung):
            em[:, (2 * i + 1) * seg:(2 * i + 2) * seg, 1 + n] += 9.6
        for i in range(len(sung) + 1):
            em[:, 2 * i * seg:(2 * i + 1) * seg, 0] += 9.6
        return em.to(dev)

    class Shape:
        """One shape's device inputs and the legs over them; every leg owns its outputs and its workspace."""

        def __init__(self, B, T, L, em):
            self.B, self.T, self.L, self.em = B, T, L, em
            self.labels = torch.arange(1, L + 1, dtype=torch.int32).repeat(B, 1).to(dev)
            self.n_labels = torch.full((B,), L, dtype=torch.int32, device=dev)
            self.n_frames = torch.full((B,), T, dtype=torch.int32, device=dev)

        def _workspace(self, L_, query):
            need = ctypes.c_size_t(0)
            assert getattr(L_, query)(self.B, self.T, self.L, ctypes.byref(need)) == 0
            return torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev), need.value

        def _inputs(self):
            em, L = self.em, self.L
            return (ptr(em), em.stride(0), em.stride(1), ptr(self.labels), L, ptr(self.n_labels), ptr(self.n_frames), self.B, self.T, L)

        def dp_leg(self, L_, stem, skip=None, windows=None):
            """stem: viterbi (plain) or viterbi_lattice -> (call, outputs (onset, offset, score, status))"""
            B, L = self.B, self.L
            ws, need = self._workspace(L_, f"la_{stem}_workspace_bytes")
            out = (torch.full((B, L), -7, dtype=torch.int32, device=dev), torch.full((B, L), -7, dtype=torch.int32, device=dev),
                   torch.full((B,), -7.0, dtype=torch.float64, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev))
            more = ()
            if stem == "viterbi_lattice":
                more = (ptr(skip), L + 1 if skip is not None else 0, 0.0) + ((ptr(windows[0]), ptr(windows[1]), 2 * L + 1) if windows is not None else (0, 0, 0))
            entry = getattr(L_, f"la_{stem}_batch")

            def fn(_held=(skip, windows)):      # `more` holds bare addresses: the leg keeps their tensors alive
                assert entry(*self._inputs(), ptr(out[0]), ptr(out[1]), L, ptr(out[2]), ptr(out[3]), *more, ptr(ws), need, stream_ptr()) == 0, _lib.last_error()
            return fn, out

        def post_leg(self, L_, stem, path, skip=None, windows=None):
            """stem: alignment_posteriors (plain), _spans, _windows or _lattice; path = the DP's (onset, offset)
            -> (call, outputs (occupancy, onset_prob, offset_prob, present_prob, span_skip_prob, log_z, status))"""
            B, L = self.B, self.L
            ws, need = self._workspace(L_, f"la_{stem}_workspace_bytes")
            f32 = lambda n: torch.full((B, n), -7.0, dtype=torch.float32, device=dev)
            out = (f32(L), f32(L), f32(L), f32(L), f32(L + 1), torch.full((B,), -7.0, dtype=torch.float64, device=dev),
                   torch.full((B,), -7, dtype=torch.int32, device=dev))
            more, span_out = (), (ptr(out[3]), ptr(out[4]))
            if stem == "alignment_posteriors":
                span_out = ()
            else:
                more = (ptr(skip), L + 1, 0.0)
            if stem in ("alignment_posteriors_windows", "alignment_posteriors_lattice"):
                more += (ptr(windows[0]), ptr(windows[1]), 2 * L + 1) if windows is not None else (0, 0, 0)
            entry = getattr(L_, f"la_{stem}")

            def fn(_held=(skip, windows, path)):
                assert entry(*self._inputs(), ptr(path[0]), ptr(path[1]), L, 2, *more, ptr(out[0]), ptr(out[1]), ptr(out[2]), *span_out,
                             ptr(out[5]), ptr(out[6]), 0, 0, 0, ptr(ws), need, stream_ptr()) == 0, _lib.last_error()
            return fn, out, need

        def open_windows(self):
            return (torch.zeros((self.B, 2 * self.L + 1), dtype=torch.int32, device=dev),
                    torch.full((self.B, 2 * self.L + 1), self.T, dtype=torch.int32, device=dev))

    def measure(title, legs):
        """legs: [(name, call, outputs)], the status the last output -> {name: (median, min, max)}; every status LA_OK"""
        for _ in range(3):
            for _, fn, _ in legs:
                fn()
        torch.cuda.synchronize()
        for name, _, out in legs:
            assert int(out[-1].abs().sum()) == 0, f"{name}: status not LA_OK"
        ts = [[] for _ in legs]
        for _ in range(args.runs):
            for i, (_, fn, _) in enumerate(legs):
                ts[i].append(_time_once(torch, fn))
        say(f"## {title}")
        return {name: (statistics.median(t), min(t), max(t)) for (name, _, _), t in zip(legs, ts)}

    def same(a, b):
        return all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))

    def against_parent(name, width, stats):
        (m, lo_t, hi_t), (pm, plo, phi) = stats[name], stats["parent commit: " + name]
        where = "inside" if plo <= m <= phi else ("BELOW" if m < plo else "ABOVE")
        say(f"{name:{width}s} {m:8.3f} ({lo_t:.3f} .. {hi_t:.3f}) against the parent's {pm:.3f} ({plo:.3f} .. {phi:.3f}): {where} its "
            f"min .. max ({100 * (m / pm - 1):+.1f} % of its median); outputs bit-equal")

    say(f"# whole-song posteriors on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a warm-up of 3, "
        f"legs alternated call by call, device events around one call, ms")
    for title, T, L in SONGS + (BITS_ONLY if parent is not None else []):
        lengths = [LINE] * (L // LINE)
        optional = [i % 4 == 3 for i in range(len(lengths))]
        sung = [n for i in range(len(lengths)) if not optional[i] for n in range(LINE * i, LINE * i + LINE)]
        sh = Shape(1, T, L, planted(1, T, L, sung, T + L))
        skip = torch.tensor([spans_from_lines(lengths, optional)], dtype=torch.int32).to(dev)
        starts = [LINE * i for i in range(len(lengths))]

        def anchored(onsets):
            """One onset anchor per line at the frame the given result has for the line's first character (a line left out: the next line's)"""
            anchors, nxt = [], None
            for a in reversed(starts):
                f = int(onsets[a])
                nxt = f if f >= 0 else nxt
                anchors.append((a, (nxt if nxt is not None else T - 1) * HOP, TOL_S))
            lo, hi = windows_from_anchors(L, T, onset_anchors=anchors)
            return torch.tensor([lo], dtype=torch.int32).to(dev), torch.tensor([hi], dtype=torch.int32).to(dev)

        plain = sh.dp_leg(lib(), "viterbi")
        sheet_only = sh.dp_leg(lib(), "viterbi_lattice", skip)
        plain[0](); sheet_only[0]()
        torch.cuda.synchronize()
        assert int(plain[1][3][0]) == 0 and int(sheet_only[1][3][0]) == 0
        lattices = [(None, None), (None, sh.open_windows()), (None, anchored(plain[1][0][0].cpu())), (skip, anchored(sheet_only[1][0][0].cpu()))]
        legs, beside = [], []
        for name, (sk, win) in zip(LATTICES, lattices):
            dp = sh.dp_leg(lib(), "viterbi_lattice", sk, win)
            dp[0]()
            torch.cuda.synchronize()
            post = sh.post_leg(lib(), "alignment_posteriors_lattice", dp[1][:2], sk, win)
            legs += [("la_viterbi_lattice_batch, " + name, dp[0], dp[1]), ("la_alignment_posteriors_lattice, " + name, post[0], post[1])]
            ws_mb = post[2] / 1e6
            if parent is not None:
                theirs = sh.post_leg(parent, "alignment_posteriors_lattice", dp[1][:2], sk, win)
                post[0](); theirs[0]()
                torch.cuda.synchronize()
                assert int(post[1][6][0]) == 0 and same(post[1], theirs[1]), f"{title}, {name}: outputs differ from the parent commit's"
                beside.append(("parent commit: la_alignment_posteriors_lattice, " + name, theirs[0], theirs[1]))
        if (title, T, L) in BITS_ONLY:
            say(f"## {title}: la_alignment_posteriors_lattice on the four lattices, all seven outputs equal the parent commit's bit for bit (not timed)")
            continue
        stats = measure(title, legs + beside)
        for i in range(0, len(legs), 2):
            (dn, (dm, dlo, dhi)), (pn, (pm, plo, phi)) = [(legs[i + j][0], stats[legs[i + j][0]]) for j in (0, 1)]
            say(f"{dn:72s} {dm:9.3f} ({dlo:.3f} .. {dhi:.3f})")
            say(f"{pn:72s} {pm:9.3f} ({plo:.3f} .. {phi:.3f})   {pm / dm:5.2f} x the DP on the same lattice")
        open_same = same(legs[1][2], legs[3][2])
        last = legs[-1][2]
        say(f"workspace {ws_mb:.0f} MB; every status LA_OK; all-open outputs equal the nothing-given ones bit for bit: {open_same}; with the sheet "
            f"{int((last[3][0] < 0.5).sum())} of {L} labels have sung_prob < 0.5, log_z {float(last[5][0]):.3f}")
        for name, _, _ in legs[1::2] if parent is not None else []:
            against_parent(name, 72, stats)
        del sh, legs, beside, plain, sheet_only, lattices
        torch.cuda.empty_cache()

    if parent is not None:
        for title, B, T, L in EXISTING:
            sh = Shape(B, T, L, planted(B, T, L, list(range(L)), B + T + L))
            none = torch.full((B, L + 1), -1, dtype=torch.int32, device=dev)
            dp = sh.dp_leg(lib(), "viterbi")
            dp[0]()
            torch.cuda.synchronize()
            names = ("la_alignment_posteriors", "la_alignment_posteriors_spans, no span", "la_alignment_posteriors_windows, all windows open")
            legs = []
            for who, L_ in (("", lib()), ("parent commit: ", parent)):
                for name, (stem, sk, win) in zip(names, (("alignment_posteriors", None, None), ("alignment_posteriors_spans", none, None),
                                                         ("alignment_posteriors_windows", None, sh.open_windows()))):
                    fn, out, _ = sh.post_leg(L_, stem, dp[1][:2], sk, win)
                    legs.append((who + name, fn, out))
            for _, fn, _ in legs:
                fn()
            torch.cuda.synchronize()
            for i in range(3):
                keep = (0, 1, 2, 5, 6) if i == 0 else range(7)         # the plain entry writes no span outputs
                assert same([legs[i][2][j] for j in keep], [legs[3 + i][2][j] for j in keep]), f"{legs[i][0]}: outputs differ from the parent commit's"
            stats = measure(title + ": the existing entries beside the parent's", legs)
            for name in names:
                against_parent(name, 52, stats)
            del sh, legs
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
