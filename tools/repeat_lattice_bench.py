"""Cost of the alignment DP with repeatable lyric lines (la_viterbi_repeats_batch; csrc/la_viterbi.hip) and what adding it did to the
existing entries.

    python tools/repeat_lattice_bench.py [--runs 30] [--parent-lib <liblyricalign_hip.so of the parent commit>] [--out profiles/repeat_lattice.txt]

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

import argparse
import ctypes
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
EXISTING = ("la_viterbi_batch", "la_viterbi_lattice_batch, nothing given", "la_viterbi_lattice_batch, every fourth line optional",
            "la_viterbi_lattice_batch, all windows open")
NEW = ("la_viterbi_repeats_batch, nothing given", "la_viterbi_repeats_batch, one repeatable chorus",
       "la_viterbi_repeats_batch, repeat span chorus .. verse + the verse optional")
SHAPES = [("32 clips x 1500 frames x 26 labels (1 wave, masks in LDS)", 32, 1500, 26),
          ("1 song x 5389 frames x 200 labels (8 waves)", 1, 5389, 200),
          ("1 song x 12000 frames x 800 labels (2 states per thread)", 1, 12000, 800),
          ("1 song x 12000 frames x 2500 labels (8 states per thread)", 1, 12000, 2500)]
LINE = 10


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
    from lyricalignment_amd.utils.alignment import repeats_from_lines, spans_from_lines
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("la_viterbi_workspace_bytes", "la_viterbi_batch", "la_viterbi_lattice_workspace_bytes", "la_viterbi_lattice_batch"):
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

    def measure(title, legs):
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
        stats = {}
        for (name, _), t in zip(legs, ts):
            stats[name] = (statistics.median(t), min(t), max(t))
            say(f"{name:86s} {stats[name][0]:8.3f} ({stats[name][1]:.3f} .. {stats[name][2]:.3f})")
        return stats

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a[:4], b[:4])) and a[2].cpu().numpy().tobytes() == b[2].cpu().numpy().tobytes()

    say(f"# alignment DP with repeatable lines on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a warm-up "
        f"of 3, legs alternated call by call, device events around one call, ms")
    for title, B, T, L in SHAPES:
        lengths = [LINE] * (L // LINE) + ([L % LINE] if L % LINE else [])
        starts = [sum(lengths[:i]) for i in range(len(lengths))]
        sung = [n for i, (a, n_chars) in enumerate(zip(starts, lengths)) for n in list(range(a, a + n_chars)) * (2 if i == 1 else 1)]
        em = planted(B, T, L, sung, B + T + L)
        labels = torch.arange(1, L + 1, dtype=torch.int32).repeat(B, 1).to(dev)
        n_labels = torch.full((B,), L, dtype=torch.int32, device=dev)
        n_frames = torch.full((B,), T, dtype=torch.int32, device=dev)
        sheet = torch.tensor([spans_from_lines(lengths, [i % 4 == 3 for i in range(len(lengths))])] * B, dtype=torch.int32).to(dev)
        verse = torch.tensor([spans_from_lines(lengths, [i == 2 for i in range(len(lengths))])] * B, dtype=torch.int32).to(dev)
        chorus = torch.tensor([repeats_from_lines(lengths, [i == 1 for i in range(len(lengths))])] * B, dtype=torch.int32).to(dev)
        both = chorus.clone()
        both[:, starts[1]] = starts[2] + lengths[2]                        # the repeat span runs over chorus .. verse
        win = (torch.zeros((B, 2 * L + 1), dtype=torch.int32, device=dev), torch.full((B, 2 * L + 1), T, dtype=torch.int32, device=dev))

        def leg(L_, stem, skip=None, windows=None, repeat=None):
            """stem: viterbi (plain), viterbi_lattice or viterbi_repeats -> (call, outputs); every leg owns its outputs and its workspace"""
            need = ctypes.c_size_t(0)
            assert getattr(L_, f"la_{stem}_workspace_bytes")(B, T, L, ctypes.byref(need)) == 0
            out = (torch.full((B, L), -7, dtype=torch.int32, device=dev), torch.full((B, L), -7, dtype=torch.int32, device=dev),
                   torch.full((B,), -7.0, dtype=torch.float64, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev),
                   torch.full((B, T), -7, dtype=torch.int32, device=dev))
            ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev)
            more = ()
            if stem != "viterbi":
                more += (ptr(skip), L + 1 if skip is not None else 0, 0.0)
                more += (ptr(windows[0]), ptr(windows[1]), 2 * L + 1) if windows is not None else (0, 0, 0)
            if stem == "viterbi_repeats":
                more += (ptr(repeat), L if repeat is not None else 0, 0.0, ptr(out[4]), T)
            entry = getattr(L_, f"la_{stem}_batch")

            def fn(_held=(skip, windows, repeat)):      # `more` holds bare addresses: the leg keeps their tensors alive
                assert entry(ptr(em), em.stride(0), em.stride(1), ptr(labels), L, ptr(n_labels), ptr(n_frames), B, T, L, ptr(out[0]),
                             ptr(out[1]), L, ptr(out[2]), ptr(out[3]), *more, ptr(ws), need.value, stream_ptr()) == 0, _lib.last_error()
            return fn, out

        def existing(L_):
            return [leg(L_, "viterbi"), leg(L_, "viterbi_lattice"), leg(L_, "viterbi_lattice", sheet), leg(L_, "viterbi_lattice", None, win)]

        legs = list(zip(EXISTING, existing(lib())))
        legs += list(zip(NEW, [leg(lib(), "viterbi_repeats"), leg(lib(), "viterbi_repeats", None, None, chorus),
                               leg(lib(), "viterbi_repeats", verse, None, both)]))
        if parent is not None:
            legs += [("parent commit: " + name, l) for name, l in zip(EXISTING, existing(parent))]
        for _, (fn, _) in legs:
            fn()
        torch.cuda.synchronize()
        assert same(legs[1][1][1], legs[4][1][1]), "la_viterbi_repeats_batch with nothing given differs from la_viterbi_lattice_batch"
        for i in range(4) if parent is not None else ():
            assert same(legs[i][1][1], legs[7 + i][1][1]), f"{legs[i][0]}: outputs differ from the parent commit's"
        visits = []
        for i in (4, 5, 6):
            p = legs[i][1][1][4][0].cpu()
            odd = p[(p % 2 == 1)]
            visits.append(int((odd[1:] != odd[:-1]).sum()) + 1)
        stats = measure(title, legs)
        say(f"visits on the reported path of clip 0: {visits[0]} with nothing repeatable, {visits[1]} with the chorus repeatable, {visits[2]} with "
            f"chorus .. verse repeatable and the verse optional ({L} labels on the sheet); nothing-given outputs equal "
            f"la_viterbi_lattice_batch's bit for bit; every status LA_OK")
        m, base = stats[NEW[0]][0], stats[EXISTING[1]][0]
        say(f"{NEW[0]}: {m:.3f} beside {EXISTING[1]} {base:.3f} of the same build ({100 * (m / base - 1):+.1f} %)")
        for name in NEW[1:]:
            say(f"{name}: {stats[name][0]:.3f} ({100 * (stats[name][0] / base - 1):+.1f} % of {EXISTING[1]})")
        for name in EXISTING if parent is not None else ():
            m, (pm, plo, phi) = stats[name][0], stats["parent commit: " + name]
            where = "inside" if plo <= m <= phi else (f"BELOW by {plo - m:.3f} ms" if m < plo else f"ABOVE by {m - phi:.3f} ms")
            say(f"{name}: {m:.3f} against the parent's {pm:.3f} ({plo:.3f} .. {phi:.3f}): {where} its min .. max ({100 * (m / pm - 1):+.1f} % of its median)")
        say()
        del legs, em
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
