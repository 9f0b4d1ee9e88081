"""Cost of the pronunciation scores (csrc/la_pronunciation.hip: la_segment_class_scores behind the lattice) alone, beside the DP on the
same lattice, and inside AlignModel.align with and without the keyword.

    python tools/pronunciation_bench.py [--runs 30] [--out profiles/pronunciation.txt]

Two shapes -- 32 clips x 1500 frames x 26 labels and 1 song x 12000 frames x 800 labels -- with 402 candidate classes (the pinyin
syllables).
Kernel legs, on synthetic emissions that plant an even segmentation, alternated call by call (caller-owned buffers, device events
around one call, a synchronise after each):
  * la_segment_class_scores on the trailing column window of the widened matrix [B, T, 1 + L + 402] and the DP's boundaries;
  * la_viterbi_batch on the leading columns of the same matrix: the DP the entry sits behind;
  * a device copy of as many bytes as the entry reads at most (every frame of every candidate column once), as one read and one write of
    half of them each: the memory system's rate for that traffic.
Model legs, a whisper-tiny-sized AlignModel with random weights (the cost does not depend on the weights), wall clock around one call
with a synchronise, alternated call by call:
  * AlignModel.align(audios, labels);
  * the same call with return_pronunciation=True, pronunciation_classes=402: the head writes 402 more emission columns per frame, the
    plain lattice's DP runs as a launch of its own, la_segment_class_scores follows, and the host formats the dicts.
Every number is the median of `runs` calls after a warm-up of 3; min .. max is printed next to it.  The entry's outputs are checked
against a float64 loop on the host (bit-equal) before anything is timed.  These numbers are recorded, not gated.
"""
from __future__ import annotations

import numpy as np
import torch

import benchlib as bl

SHAPES = [("32 clips x 1500 frames x 26 labels", 32, 1500, 26), ("1 song x 12000 frames x 800 labels", 1, 12000, 800)]
N_CAND, TOP_K = 402, 5


def main(argv=None):
    args = bl.parse(bl.parser(), argv)
    report = bl.Report(args.out)
    say = report.say
    dev, lib = bl.open_gpu()
    from lyricalignment_amd import _lib, ops, whisper_compat as wc
    from lyricalignment_amd._lib import ptr, stream_ptr
    from lyricalignment_amd.module.align_model import AlignModel
    say(f"# pronunciation scores on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.runs} calls after a warm-up of 3, legs "
        f"alternated call by call, ms; {N_CAND} candidate classes, top_k {TOP_K}")
    say("# kernel legs: device events around one call")
    for title, B, T, L in SHAPES:
        g = torch.Generator().manual_seed(B + T + L)
        W = 1 + L + N_CAND
        em_w = -torch.rand((B, T, W), generator=g) * 12 - 1                # planted as tools/wide_lattice_bench.py plants
        seg = T // (2 * L + 1)
        for n in range(L):
            em_w[:, (2 * n + 1) * seg:(2 * n + 2) * seg, 1 + n] += 9.6
            em_w[:, (2 * n + 1) * seg:(2 * n + 2) * seg, 1 + L + (7 * n) % N_CAND] += 9.6        # the class heard there
        for i in range(L + 1):
            em_w[:, 2 * i * seg:(2 * i + 1) * seg, 0] += 9.6
        em_h = em_w
        em_w = em_w.to(dev)
        em, em_c = em_w[:, :, : 1 + L], em_w[:, :, 1 + L:]
        labels = torch.arange(1, L + 1, dtype=torch.int32, device=dev)[None].repeat(B, 1)
        n_lab = torch.full((B,), L, dtype=torch.int32, device=dev)
        nf = torch.full((B,), T, dtype=torch.int32, device=dev)
        own = ((7 * torch.arange(L, dtype=torch.int32)) % N_CAND)[None].repeat(B, 1)
        own[:, 0::4] = (own[:, 0::4] + 1) % N_CAND                          # every fourth position: the sheet names another class
        own = own.to(dev)
        onset, offset, _, status = ops.viterbi_batch(em, labels, n_lab, nf)
        top_col, top_score, own_score, own_rank, n_seg = ops.segment_class_scores(em_c, n_lab, onset, offset, own, TOP_K)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        on_h, off_h = onset[0].cpu().numpy(), offset[0].cpu().numpy()       # clip 0 against a float64 loop on the host: bit-equal
        for n in range(0, L, max(1, L // 13)):
            acc = np.zeros(N_CAND)
            for t in range(on_h[n], off_h[n]):
                acc = acc + em_h[0, t, 1 + L:].numpy().astype(np.float64)
            order = sorted(range(N_CAND), key=lambda j: (-acc[j], j))
            assert top_col[0, n].tolist() == order[:TOP_K] and top_score[0, n].tolist() == [acc[j] for j in order[:TOP_K]], n
            assert float(own_score[0, n]) == acc[int(own[0, n])] and int(own_rank[0, n]) == order.index(int(own[0, n]))
        n_bytes = B * T * N_CAND * 4                                        # every frame of every candidate column, read once at most
        src = torch.empty((n_bytes // 2,), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def scores():
            _lib.check(lib.la_segment_class_scores(ptr(em_c), em_c.stride(0), em_c.stride(1), ptr(n_lab), ptr(onset), ptr(offset), L, ptr(own),
                                                     L, B, T, L, N_CAND, TOP_K, 0, 0, 0, ptr(top_col), ptr(top_score), TOP_K, ptr(own_score),
                                                     ptr(own_rank), ptr(n_seg), stream_ptr()), "scores")

        legs = [("la_segment_class_scores", scores), ("la_viterbi_batch on the leading columns", lambda: ops.viterbi_batch(em, labels, n_lab, nf)),
                (f"device copy of {n_bytes // 2} bytes (read + write = the entry's largest traffic)", lambda: dst.copy_(src))]
        stats = bl.stats_of(bl.alternated(legs, args.runs))
        read = int(n_seg.sum()) * N_CAND * 4
        say(f"## {title}: {int(n_seg.sum())} of {B * T} frames lie in a segment, {read / 1e6:.2f} MB read")
        for name, st in stats.items():
            say(bl.timed(name, st, 84, 8, 4))
        med = [st[0] for st in stats.values()]
        say(f"the entry reads {read / (med[0] * 1e-3) / 1e9:.1f} GB/s (copy: {n_bytes / (med[2] * 1e-3) / 1e9:.1f} GB/s) and costs "
            f"{100 * med[0] / med[1]:.1f} % of the DP; rank > 0 at {int((own_rank[0] > 0).sum())} of {L} positions of clip 0")

    say("# model legs: whisper-tiny-sized AlignModel, random weights, wall clock around one call with a synchronise")
    dims = wc.dims_for("tiny")
    model = AlignModel(wc.build_model("tiny", seed=3), embed_dim=dims.n_audio_state, hidden_dim=384, output_dim=N_CAND + 2, device="cuda:0",
                       compute_dtype=torch.bfloat16).eval()
    rs = np.random.RandomState(0)
    for title, B, T, L in SHAPES:
        audios = [(rs.randn(T * 320) * 0.1).astype(np.float32) for _ in range(B)]          # 20 ms per frame at 16 kHz
        labels = torch.from_numpy(rs.randint(1, N_CAND + 1, size=(B, L)))
        kw = dict(return_pronunciation=True, pronunciation_classes=N_CAND, pronunciation_top_k=TOP_K)
        with torch.no_grad():
            plain = model.align(audios, labels)
            seconds, pron = model.align(audios, labels, **kw)
            assert seconds == plain
            legs = [("AlignModel.align", lambda: model.align(audios, labels)),
                    ("AlignModel.align(return_pronunciation=True, pronunciation_classes=402)", lambda: model.align(audios, labels, **kw))]
            stats = bl.stats_of(bl.alternated(legs, args.runs, bl.wall_once))
        say(f"## {title}")
        for name, st in stats.items():
            say(bl.timed(name, st, 84))
        med = [st[0] for st in stats.values()]
        say(f"the keyword adds {med[1] - med[0]:.3f} ms ({100 * (med[1] - med[0]) / med[0]:.1f} %)")
    report.close()
    return report.lines


if __name__ == "__main__":
    main()
