"""Cost of the posteriors on the lattice with repeatable lyric lines (la_alignment_posteriors_repeats; the REP face of posterior_kernel in
csrc/la_posterior.hip) and what adding it did to the existing posterior entries.

    python tools/repeat_confidence_bench.py [--runs 30] [--parent-lib <liblyricalign_hip.so of the parent commit>] [--out profiles/repeat_confidence.txt]

Two shapes on synthetic emissions -- 32 clips x 1500 frames x 26 labels (one wave) and one song of 5389 frames x 200 labels (8 waves) -- in
lines of 10 labels; the emissions plant the sheet with its second line (the chorus) sung twice.  Legs, alternated call by call
(caller-owned buffers, device events around one call, a synchronise after each; no gamma output):
  * the four existing entries: la_alignment_posteriors; la_alignment_posteriors_spans with every fourth line optional;
    la_alignment_posteriors_windows with every window open; la_alignment_posteriors_lattice with nothing given.  With --parent-lib the
    parent commit's same four legs run in the same alternation (outputs checked bit for bit against this build's) and every leg's median
    is reported against the parent's own min .. max of that leg: the project's noise yardstick;
  * la_alignment_posteriors_repeats with nothing repeatable and every window open (outputs checked bit for bit against
    la_alignment_posteriors_windows'), beside la_alignment_posteriors_windows of the same build;
  * la_alignment_posteriors_repeats with the chorus repeatable, with and without path_prob: reported;
  * the loops of a clip with a jump, old face beside new: la_alignment_posteriors_windows and la_alignment_posteriors_repeats (nothing
    repeatable) with the third line optional and every window open (outputs checked bit for bit): reported.
Every posterior leg is asked about the onset / offset (and path) that la_viterbi_repeats_batch reports for its lattice.  Every number is
the median of `runs` calls after a warm-up; min .. max is printed next to it.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
EXISTING = ("la_alignment_posteriors", "la_alignment_posteriors_spans, every fourth line optional",
            "la_alignment_posteriors_windows, all windows open", "la_alignment_posteriors_lattice, nothing given")
NEW = ("la_alignment_posteriors_repeats, nothing repeatable, all windows open", "la_alignment_posteriors_repeats, one repeatable chorus",
       "la_alignment_posteriors_repeats, one repeatable chorus, with path_prob",
       "la_alignment_posteriors_windows, the third line optional, all windows open",
       "la_alignment_posteriors_repeats, the third line optional, nothing repeatable, all windows open")
SHAPES = [("32 clips x 1500 frames x 26 labels (1 wave)", 32, 1500, 26), ("1 song x 5389 frames x 200 labels (8 waves)", 1, 5389, 200)]
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
    from lyricalignment_amd import _lib, ops
    from lyricalignment_amd._lib import SYMBOLS, lib, ptr, stream_ptr
    from lyricalignment_amd.utils.alignment import repeats_from_lines, spans_from_lines
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    stems = ("alignment_posteriors", "alignment_posteriors_spans", "alignment_posteriors_windows", "alignment_posteriors_lattice")
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for stem in stems:
            for name in (f"la_{stem}_workspace_bytes", f"la_{stem}"):
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

    say(f"# posteriors on the lattice with repeatable lines on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a "
        f"warm-up of 3, legs alternated call by call, device events around one call, ms")
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
        win = (torch.zeros((B, 2 * L + 1), dtype=torch.int32, device=dev), torch.full((B, 2 * L + 1), T, dtype=torch.int32, device=dev))

        def leg(L_, stem, skip=None, windows=None, repeat=None, with_path=False):
            """-> (call, outputs); every leg owns its outputs and its workspace and asks about its own lattice's DP result"""
            dp = ops.viterbi_repeats_batch(em, labels, n_labels, n_frames, skip, 0.0, *(windows or (None, None)), repeat, 0.0)
            assert int(dp[3].abs().sum()) == 0
            need = ctypes.c_size_t(0)
            assert getattr(L_, f"la_{stem}_workspace_bytes")(B, T, L, ctypes.byref(need)) == 0
            f32 = lambda *shape: torch.full(shape, -7.0, dtype=torch.float32, device=dev)
            out = dict(occupancy=f32(B, L), onset_prob=f32(B, L), offset_prob=f32(B, L), present=f32(B, L), span_skip=f32(B, L + 1),
                       repeat_count=f32(B, L), path_prob=f32(B, T), log_z=torch.full((B,), -7.0, dtype=torch.float64, device=dev),
                       status=torch.full((B,), -7, dtype=torch.int32, device=dev))
            ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev)
            more = ()
            if stem != "alignment_posteriors":
                more += (ptr(skip), L + 1, 0.0)
            if stem in ("alignment_posteriors_windows", "alignment_posteriors_lattice", "alignment_posteriors_repeats"):
                more += (ptr(windows[0]), ptr(windows[1]), 2 * L + 1) if windows is not None else (0, 0, 0)
            outs = (ptr(out["occupancy"]), ptr(out["onset_prob"]), ptr(out["offset_prob"]))
            if stem == "alignment_posteriors_repeats":
                more += (ptr(repeat), L if repeat is not None else 0, 0.0, ptr(dp[4]) if with_path else 0, T if with_path else 0)
                outs += (ptr(out["present"]), ptr(out["span_skip"]), ptr(out["repeat_count"]), ptr(out["path_prob"]) if with_path else 0)
            elif stem != "alignment_posteriors":
                outs += (ptr(out["present"]), ptr(out["span_skip"]))
            entry = getattr(L_, f"la_{stem}")

            def fn(_held=(skip, windows, repeat, dp)):      # `more` holds bare addresses: the leg keeps their tensors alive
                assert entry(ptr(em), em.stride(0), em.stride(1), ptr(labels), L, ptr(n_labels), ptr(n_frames), B, T, L, ptr(dp[0]), ptr(dp[1]),
                             L, 2, *more, *outs, ptr(out["log_z"]), ptr(out["status"]), 0, 0, 0, ptr(ws), need.value, stream_ptr()) == 0, _lib.last_error()
            return fn, out

        def existing(L_):
            return [leg(L_, stems[0]), leg(L_, stems[1], sheet), leg(L_, stems[2], None, win), leg(L_, stems[3])]

        def same(a, b, keys):
            return all(a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() for k in keys)

        common = ("occupancy", "onset_prob", "offset_prob", "log_z", "status")
        legs = list(zip(EXISTING, existing(lib())))
        legs += list(zip(NEW, [leg(lib(), "alignment_posteriors_repeats", None, win), leg(lib(), "alignment_posteriors_repeats", None, None, chorus),
                               leg(lib(), "alignment_posteriors_repeats", None, None, chorus, True),
                               leg(lib(), "alignment_posteriors_windows", verse, win), leg(lib(), "alignment_posteriors_repeats", verse, win)]))
        if parent is not None:
            legs += [("parent commit: " + name, l) for name, l in zip(EXISTING, existing(parent))]
        for _ in range(3):
            for _, (fn, _) in legs:
                fn()
        torch.cuda.synchronize()
        for name, (_, out) in legs:
            assert int(out["status"].abs().sum()) == 0, f"{name}: status not LA_OK"
        assert same(legs[2][1][1], legs[4][1][1], common + ("present", "span_skip")), "nothing repeatable differs from la_alignment_posteriors_windows"
        assert int(legs[4][1][1]["repeat_count"].abs().sum()) == 0
        assert same(legs[7][1][1], legs[8][1][1], common + ("present", "span_skip")), "one optional line: the new face differs from the old"
        for i in range(4) if parent is not None else ():
            assert same(legs[i][1][1], legs[9 + i][1][1], common + (("present", "span_skip") if i else ())), f"{legs[i][0]}: outputs differ from the parent commit's"
        ts = [[] for _ in legs]
        for _ in range(args.runs):
            for i, (_, (fn, _)) in enumerate(legs):
                ts[i].append(_time_once(torch, fn))
        say(f"## {title}")
        stats = {}
        for (name, _), t in zip(legs, ts):
            stats[name] = (statistics.median(t), min(t), max(t))
            say(f"{name:86s} {stats[name][0]:8.3f} ({stats[name][1]:.3f} .. {stats[name][2]:.3f})")
        rc, vis = legs[5][1][1]["repeat_count"][0], legs[5][1][1]["present"][0]
        say(f"clip 0 with the chorus repeatable: repeat_count of the chorus {float(rc[starts[1]]):.4f}, visits of its first label "
            f"{float(vis[starts[1]]):.4f}, of the label after it {float(vis[starts[2]]):.4f}; nothing-repeatable outputs equal "
            f"la_alignment_posteriors_windows' bit for bit; every status LA_OK")
        m, base = stats[NEW[0]][0], stats[EXISTING[2]][0]
        say(f"{NEW[0]}: {m:.3f} beside {EXISTING[2]} {base:.3f} of the same build ({100 * (m / base - 1):+.1f} %)")
        m, base2 = stats[NEW[4]][0], stats[NEW[3]][0]
        say(f"{NEW[4]}: {m:.3f} beside {NEW[3]} {base2:.3f} ({100 * (m / base2 - 1):+.1f} %), outputs equal bit for bit")
        for name in NEW[1:3]:
            say(f"{name}: {stats[name][0]:.3f} ({100 * (stats[name][0] / base - 1):+.1f} % of {EXISTING[2]})")
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
