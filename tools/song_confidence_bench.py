"""Cost of the whole-song confidence for repeated lyric lines (la_alignment_posteriors_song; beyond 511 labels the REP face of
posterior_strip_kernel in csrc/la_posterior.hip) beside la_alignment_posteriors_lattice.

    python tools/song_confidence_bench.py [--runs 30] [--out profiles/song_confidence.txt]

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

import argparse
import ctypes
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LEGS = ("la_alignment_posteriors_lattice, nothing given",
        "la_alignment_posteriors_song, nothing repeatable",
        "la_alignment_posteriors_song, one repeatable chorus",
        "la_alignment_posteriors_lattice, one anchor per line, every fourth line optional",
        "la_alignment_posteriors_song, nothing repeatable, one anchor per line, every fourth line optional",
        "la_alignment_posteriors_song, one repeatable chorus, one anchor per line, every fourth line optional")
SONGS = [("1 song x 12000 frames x 800 labels (R = 2)", 12000, 800), ("1 song x 12000 frames x 2500 labels (R = 8)", 12000, 2500)]
LINE, HOP, TOL_S = 10, 0.02, 1.0


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
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    sys.path.insert(0, os.path.join(HERE, ".."))
    import torch
    from lyricalignment_amd import _lib, ops
    from lyricalignment_amd._lib import lib, ptr, stream_ptr
    from lyricalignment_amd.utils.alignment import repeats_from_lines, spans_from_lines, windows_from_anchors
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    B = 1

    say(f"# whole-song posteriors on the lattice with repeatable lines on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} "
        f"calls after a warm-up of 3, legs alternated call by call, device events around one call, ms")
    for title, T, L in SONGS:
        lengths = [LINE] * (L // LINE) + ([L % LINE] if L % LINE else [])
        starts = [sum(lengths[:i]) for i in range(len(lengths))]
        sung = [n for i, (a, n_chars) in enumerate(zip(starts, lengths)) for n in list(range(a, a + n_chars)) * (2 if i == 1 else 1)]
        # emissions -rand * 12 - 1 with a 0.8 * 12 bonus on an even segmentation of the SUNG labels
        g = torch.Generator().manual_seed(T + L)
        em = -torch.rand((B, T, L + 1), generator=g) * 12 - 1
        seg = T // (2 * len(sung) + 1)
        for i, n in enumerate(sung):
            em[:, (2 * i + 1) * seg:(2 * i + 2) * seg, 1 + n] += 9.6
        for i in range(len(sung) + 1):
            em[:, 2 * i * seg:(2 * i + 1) * seg, 0] += 9.6
        em = em.to(dev)
        labels = torch.arange(1, L + 1, dtype=torch.int32).repeat(B, 1).to(dev)
        n_labels = torch.full((B,), L, dtype=torch.int32, device=dev)
        n_frames = torch.full((B,), T, dtype=torch.int32, device=dev)
        sheet = torch.tensor([spans_from_lines(lengths, [i % 4 == 3 for i in range(len(lengths))])] * B, dtype=torch.int32).to(dev)
        chorus = torch.tensor([repeats_from_lines(lengths, [i == 1 for i in range(len(lengths))])] * B, dtype=torch.int32).to(dev)
        # one onset anchor per line where the planting begins the line's FIRST visit
        anchors = [(a, (2 * sung.index(a) + 1) * seg * HOP, TOL_S) for a in starts]
        lo, hi = windows_from_anchors(L, T, onset_anchors=anchors)
        win = (torch.tensor([lo] * B, dtype=torch.int32).to(dev), torch.tensor([hi] * B, dtype=torch.int32).to(dev))

        def leg(stem, skip=None, windows=None, repeat=None):
            """-> (call, outputs); every leg owns its outputs and its workspace and asks about its own lattice's DP result"""
            dp = ops.viterbi_repeats_batch(em, labels, n_labels, n_frames, skip, 0.0, *(windows or (None, None)), repeat, 0.0)
            assert int(dp[3].abs().sum()) == 0
            need = ctypes.c_size_t(0)
            assert getattr(lib(), f"la_{stem}_workspace_bytes")(B, T, L, ctypes.byref(need)) == 0
            f32 = lambda *shape: torch.full(shape, -7.0, dtype=torch.float32, device=dev)
            out = dict(occupancy=f32(B, L), onset_prob=f32(B, L), offset_prob=f32(B, L), present=f32(B, L), span_skip=f32(B, L + 1),
                       repeat_count=f32(B, L), path_prob=f32(B, T), log_z=torch.full((B,), -7.0, dtype=torch.float64, device=dev),
                       status=torch.full((B,), -7, dtype=torch.int32, device=dev))
            ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev)
            more = (ptr(skip), L + 1, 0.0) + ((ptr(windows[0]), ptr(windows[1]), 2 * L + 1) if windows is not None else (0, 0, 0))
            outs = (ptr(out["occupancy"]), ptr(out["onset_prob"]), ptr(out["offset_prob"]), ptr(out["present"]), ptr(out["span_skip"]))
            if stem == "alignment_posteriors_song":
                more += (ptr(repeat), L if repeat is not None else 0, 0.0, ptr(dp[4]), T)
                outs += (ptr(out["repeat_count"]), ptr(out["path_prob"]))
            entry = getattr(lib(), f"la_{stem}")

            def fn(_held=(skip, windows, repeat, dp)):      # `more` holds bare addresses: the leg keeps their tensors alive
                assert entry(ptr(em), em.stride(0), em.stride(1), ptr(labels), L, ptr(n_labels), ptr(n_frames), B, T, L, ptr(dp[0]), ptr(dp[1]),
                             L, 2, *more, *outs, ptr(out["log_z"]), ptr(out["status"]), 0, 0, 0, ptr(ws), need.value, stream_ptr()) == 0, _lib.last_error()
            return fn, out

        def same(a, b, keys):
            return all(a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() for k in keys)

        legs = list(zip(LEGS, [leg("alignment_posteriors_lattice"), leg("alignment_posteriors_song"),
                               leg("alignment_posteriors_song", None, None, chorus), leg("alignment_posteriors_lattice", sheet, win),
                               leg("alignment_posteriors_song", sheet, win), leg("alignment_posteriors_song", sheet, win, chorus)]))
        for _ in range(3):
            for _, (fn, _) in legs:
                fn()
        torch.cuda.synchronize()
        for name, (_, out) in legs:
            assert int(out["status"].abs().sum()) == 0, f"{name}: status not LA_OK"
        shared = ("occupancy", "onset_prob", "offset_prob", "log_z", "status", "present", "span_skip")
        assert same(legs[0][1][1], legs[1][1][1], shared) and same(legs[3][1][1], legs[4][1][1], shared), "nothing repeatable differs from the lattice entry"
        assert int(legs[1][1][1]["repeat_count"].abs().sum()) == 0 and int(legs[4][1][1]["repeat_count"].abs().sum()) == 0
        ts = [[] for _ in legs]
        for _ in range(args.runs):
            for i, (_, (fn, _)) in enumerate(legs):
                ts[i].append(_time_once(torch, fn))
        say(f"## {title}")
        stats = {}
        for (name, _), t in zip(legs, ts):
            stats[name] = (statistics.median(t), min(t), max(t))
            say(f"{name:100s} {stats[name][0]:9.3f} ({stats[name][1]:.3f} .. {stats[name][2]:.3f})")
        for i in (2, 5):
            rc, vis = legs[i][1][1]["repeat_count"][0], legs[i][1][1]["present"][0]
            say(f"{LEGS[i]}: repeat_count of the chorus {float(rc[starts[1]]):.4f}, visits of its first label {float(vis[starts[1]]):.4f}, "
                f"of the label after it {float(vis[starts[2]]):.4f}")
        say("nothing-repeatable outputs equal la_alignment_posteriors_lattice's bit for bit on both lattices; every status LA_OK")
        for i, base in ((1, 0), (2, 0), (4, 3), (5, 3)):
            m, b0 = stats[LEGS[i]][0], stats[LEGS[base]][0]
            say(f"{LEGS[i]}: {m:.3f} beside {LEGS[base]} {b0:.3f} ({100 * (m / b0 - 1):+.1f} %)")
        say()
        del legs, em
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
