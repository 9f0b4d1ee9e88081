"""Cost of the strip kernel's span and window faces (la_viterbi_lattice_batch beyond 511 labels) beside the plain strip kernel
(la_viterbi_batch) at the same shape; csrc/la_viterbi.hip.

    python tools/wide_lattice_bench.py [--runs 30] [--parent-lib <liblyricalign_hip.so of the parent commit>] [--out profiles/wide_lattice.txt]

Two whole songs on synthetic emissions -- 12000 frames x 800 labels (2 states per thread) and 12000 frames x 2500 labels (8 states per
thread), both in lines of 10 labels with every fourth line optional; the emissions plant the mandatory lines.
Legs, alternated call by call (caller-owned buffers, device events around one call, a synchronise after each):
  * la_viterbi_batch: the plain strip kernel, the yardstick;
  * la_viterbi_lattice_batch with nothing given (the same kernel through the general entry);
  * la_viterbi_lattice_batch with every window [0, T) and a null skip_from: what the window face costs when nothing is known;
  * la_viterbi_lattice_batch with one onset anchor per line (the line's first character within 1 s of where the unanchored DP put it);
  * la_viterbi_lattice_batch with anchors (around the sheet-only DP's result) and every fourth line optional.
With --parent-lib the parent commit's five legs run in the same alternation (outputs checked bit for bit against this build's), and at
32 clips x 1500 frames x 26 labels the parent's la_viterbi_batch, span-free la_viterbi_spans_batch and all-open la_viterbi_windows_batch
run beside this build's: every leg's median is reported against the parent's min .. max of the same leg.
Every number is the median of `runs` calls after a warm-up; min .. max is printed next to it.  The nothing-given and all-open outputs are
checked bit for bit against la_viterbi_batch's, and every leg's status is LA_OK, before anything is timed.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SONG_LEGS = ("la_viterbi_batch", "la_viterbi_lattice_batch, nothing given", "la_viterbi_lattice_batch, all windows open",
             "la_viterbi_lattice_batch, one onset anchor per line, +-1 s", "la_viterbi_lattice_batch, anchors + every fourth line optional")
SONGS = [("1 song x 12000 frames x 800 labels (2 states per thread)", 12000, 800),
         ("1 song x 12000 frames x 2500 labels (8 states per thread)", 12000, 2500)]
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
        for name in ("la_viterbi_workspace_bytes", "la_viterbi_batch", "la_viterbi_spans_workspace_bytes", "la_viterbi_spans_batch",
                     "la_viterbi_windows_workspace_bytes", "la_viterbi_windows_batch", "la_viterbi_lattice_workspace_bytes",
                     "la_viterbi_lattice_batch"):
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

        def _buffers(self, L_, query):
            B, T, L = self.B, self.T, self.L
            need = ctypes.c_size_t(0)
            assert getattr(L_, query)(B, T, L, ctypes.byref(need)) == 0
            out = (torch.full((B, L), -7, dtype=torch.int32, device=dev), torch.full((B, L), -7, dtype=torch.int32, device=dev),
                   torch.full((B,), -7.0, dtype=torch.float64, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev))
            return out, torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev), need.value

        def _head(self, out):
            B, T, L, em = self.B, self.T, self.L, self.em
            return (ptr(em), em.stride(0), em.stride(1), ptr(self.labels), L, ptr(self.n_labels), ptr(self.n_frames), B, T, L,
                    ptr(out[0]), ptr(out[1]), L, ptr(out[2]), ptr(out[3]))

        def leg(self, L_, stem, skip=None, windows=None):
            """stem: viterbi (plain), viterbi_spans, viterbi_windows or viterbi_lattice -> (call, outputs)"""
            out, ws, need = self._buffers(L_, f"la_{stem}_workspace_bytes")
            L = self.L
            more = ()
            if stem != "viterbi":
                more += (ptr(skip), L + 1 if skip is not None else 0, 0.0)
            if stem in ("viterbi_windows", "viterbi_lattice"):
                more += (ptr(windows[0]), ptr(windows[1]), 2 * L + 1) if windows is not None else (0, 0, 0)
            entry = getattr(L_, f"la_{stem}_batch")

            def fn(_held=(skip, windows)):      # `more` holds bare addresses: the leg keeps their tensors alive
                assert entry(*self._head(out), *more, ptr(ws), need, stream_ptr()) == 0, _lib.last_error()
            return fn, out

        def open_windows(self):
            return (torch.zeros((self.B, 2 * self.L + 1), dtype=torch.int32, device=dev),
                    torch.full((self.B, 2 * self.L + 1), self.T, dtype=torch.int32, device=dev))

    def measure(title, legs, yardstick=0):
        for _ in range(3):
            for _, (fn, _) in legs:
                fn()
        torch.cuda.synchronize()
        for name, (_, out) in legs:
            assert int(out[3].abs().sum()) == 0, f"{name}: status not LA_OK"
        ts = [[] for _ in legs]
        for _ in range(args.runs):
            for i, (_, (fn, _)) in enumerate(legs):
                ts[i].append(_time_once(torch, fn))
        say(f"## {title}")
        base = statistics.median(ts[yardstick])
        stats = {}
        for (name, _), t in zip(legs, ts):
            m, lo_t, hi_t = statistics.median(t), min(t), max(t)
            stats[name] = (m, lo_t, hi_t)
            say(f"{name:66s} {m:8.3f} ({lo_t:.3f} .. {hi_t:.3f})   {m / base:5.2f} x la_viterbi_batch")
        return stats

    def against_parent(stats, name):
        m, (pm, plo, phi) = stats[name][0], stats["parent commit: " + name]
        where = "inside" if plo <= m <= phi else ("BELOW" if m < plo else "ABOVE")
        say(f"{name}: {m:.3f} against the parent's {pm:.3f} ({plo:.3f} .. {phi:.3f}): {where} its min .. max "
            f"({100 * (m / pm - 1):+.1f} % of its median)")

    def same(a, b):
        diff = [f"{name}: {int((x != y).sum())} of {x.numel()}" for name, x, y in zip(("onset", "offset", "score", "status"), a, b) if not torch.equal(x, y)]
        if diff:
            print("outputs differ -- " + "; ".join(diff), flush=True)
        return not diff

    say(f"# whole-song alignment lattices on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a warm-up of 3, "
        f"legs alternated call by call, device events around one call, ms")
    for title, T, L in SONGS:
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

        plain = sh.leg(lib(), "viterbi")
        sheet_only = sh.leg(lib(), "viterbi_lattice", skip)
        plain[0](); sheet_only[0]()
        torch.cuda.synchronize()
        assert int(plain[1][3][0]) == 0 and int(sheet_only[1][3][0]) == 0
        win_a, win_s = anchored(plain[1][0][0].cpu()), anchored(sheet_only[1][0][0].cpu())

        def song_legs(L_, first):
            return [first, sh.leg(L_, "viterbi_lattice"), sh.leg(L_, "viterbi_lattice", None, sh.open_windows()),
                    sh.leg(L_, "viterbi_lattice", None, win_a), sh.leg(L_, "viterbi_lattice", skip, win_s)]

        legs = list(zip(SONG_LEGS, song_legs(lib(), plain)))
        if parent is not None:
            legs += [("parent commit: " + name, leg) for name, leg in zip(SONG_LEGS, song_legs(parent, sh.leg(parent, "viterbi")))]
        for _, (fn, _) in legs:
            fn()
        torch.cuda.synchronize()
        for i in (1, 2) + ((5, 6, 7) if parent is not None else ()):
            assert same(legs[0][1][1], legs[i][1][1]), f"{legs[i][0]}: outputs differ from la_viterbi_batch"
        for i in (3, 4) if parent is not None else ():
            assert same(legs[i][1][1], legs[5 + i][1][1]), f"{legs[i][0]}: outputs differ from the parent commit's"
        kept = same(legs[0][1][1], legs[3][1][1]), same(sheet_only[1], legs[4][1][1])      # the anchors lie around each DP's own result
        stats = measure(title, legs)
        left = int((legs[4][1][1][0][0] < 0).sum())
        closed = float(((win_a[0] > 0) | (win_a[1] < T)).float().mean())
        say(f"nothing-given and all-open outputs equal la_viterbi_batch's bit for bit; anchors narrow {100 * closed:.0f} % of the states' windows; "
            f"every status LA_OK; the sheet leaves {left} of {L} labels out; anchored result equals the unanchored one: {kept[0]}, with the "
            f"sheet: {kept[1]}")
        if parent is not None:
            for name in SONG_LEGS:
                against_parent(stats, name)
        del sh, legs, plain, sheet_only
        torch.cuda.empty_cache()

    if parent is not None:
        B, T, L = 32, 1500, 26
        sh = Shape(B, T, L, planted(B, T, L, list(range(L)), B + T + L))
        none = torch.full((B, L + 1), -1, dtype=torch.int32, device=dev)
        names = ("la_viterbi_batch", "la_viterbi_spans_batch, no span", "la_viterbi_windows_batch, all windows open")
        legs = []
        for who, L_ in (("", lib()), ("parent commit: ", parent)):
            legs += [(who + names[0], sh.leg(L_, "viterbi")), (who + names[1], sh.leg(L_, "viterbi_spans", none)),
                     (who + names[2], sh.leg(L_, "viterbi_windows", None, sh.open_windows()))]
        for _, (fn, _) in legs:
            fn()
        torch.cuda.synchronize()
        for name, (_, out) in legs[1:]:
            assert same(legs[0][1][1], out), f"{name}: outputs differ from la_viterbi_batch"
        stats = measure("32 clips x 1500 frames x 26 labels (1 wave, masks in LDS): the existing entries beside the parent's", legs)
        for name in names:
            against_parent(stats, name)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
