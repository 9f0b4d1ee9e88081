"""Short utterances of different lengths through harness.align_records at batch_size 1, 8, 32 (AlignModel.align(per_clip=True)).

    python tools/ragged_batch_bench.py [--clips 206] [--batch-sizes 1,8,32] [--passes 5] [--dtype bfloat16] [--model medium] [--out FILE]

206 synthetic clips with seeded lengths uniform in 0.8-7.9 s and 1-26 labels (the size and the ranges of Opencpop's test split),
Whisper-medium with random-init weights, bfloat16.  Per batch size: one warm-up pass over all clips, then `passes` timed passes (host wall
clock around the whole pass with a device synchronise at its end: tokenising, sorting, padding, the host-to-device copies and the result
copies are part of what a user waits for); the median pass is reported as clips per second and milliseconds per clip.  batch_size = 1 is
the path as it was before the per-clip mode existed (one record per device call) and the baseline of the same run on the same box.
With --stages the per-stage device times of one batch of the largest size (log-mel, encoder, head + DP) are printed too.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

VOCAB = 21129


class Record:
    def __init__(self, audio, text):
        self.audio, self.text = audio, text


def _wave(n, seed):
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    f = 180.0 + 3.0 * (seed % 97)
    return (rs.randn(n) * 0.05 + 0.3 * np.sin(2 * np.pi * f * t) + 0.2 * np.sin(2 * np.pi * 2500 * t * (1 + 0.1 * t))).astype(np.float32)


def make_records(n_clips, seed=0):
    rs = np.random.RandomState(seed)
    secs = rs.uniform(0.8, 7.9, size=n_clips)
    n_lab = rs.randint(1, 27, size=n_clips)
    records, ids = [], {}
    for i in range(n_clips):
        # at most one label per 3 output frames, so that every synthetic clip has a feasible CTC lattice
        L = int(min(n_lab[i], max(1, int(secs[i] * 50) // 3)))
        text = "".join(chr(0x4E00 + (i * 31 + j) % 20000) for j in range(L))
        ids.setdefault(text, [int(v) for v in rs.randint(2, 403, size=L)])
        records.append(Record(_wave(int(secs[i] * 16000), i), text))
    return records, ids, secs


def _event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=206)
    ap.add_argument("--batch-sizes", default="1,8,32")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--dtype", default="bfloat16")
    ap.add_argument("--model", default="medium")
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from lyricalignment_amd import _lib, whisper_compat as wc
    from lyricalignment_amd.harness import PinyinClassLUT, align_records
    from lyricalignment_amd.module.align_model import AlignModel
    _lib.require_gpu()
    torch.cuda.set_device(0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dtype = getattr(torch, args.dtype)
    dims = wc.dims_for(args.model)
    model = AlignModel(wc.build_model(args.model, seed=3), embed_dim=dims.n_audio_state, hidden_dim=384, output_dim=VOCAB, device="cuda:0",
                       compute_dtype=dtype).eval()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n, p in model.align_rnn.named_parameters():
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * ((12.0 if n.startswith("fc.weight") else 1.5) / 384 ** 0.5))
    records, ids, secs = make_records(args.clips)
    by_text = ids
    lut = PinyinClassLUT([str(i) for i in range(VOCAB)], {str(i): i for i in range(VOCAB)})
    tokenize = lambda t: by_text[t]
    sizes = [int(b) for b in args.batch_sizes.split(",")]
    say(f"# Whisper-{args.model} {args.dtype}, {torch.cuda.get_device_name(0)}; {args.clips} clips of {secs.min():.2f}-{secs.max():.2f} s "
        f"(mean {secs.mean():.2f} s, {secs.sum():.0f} s of audio), 1-26 labels; harness.align_records, 1 warm-up + median of {args.passes} passes")
    say(f"{'batch_size':>10} {'pass s':>8} {'clips/s':>9} {'ms/clip':>8} {'x realtime':>10} {'vs batch_size 1':>15}   passes (s)")
    results, base = {}, None
    for bs in sizes:
        results[bs] = align_records(model, records, lut, tokenize, use_ctc_loss=True, batch_size=bs)      # warm-up
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.passes):
            t0 = time.perf_counter()
            align_records(model, records, lut, tokenize, use_ctc_loss=True, batch_size=bs)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        med = statistics.median(ts)
        base = med if base is None and bs == 1 else base
        rel = f"{base / med:>14.2f}x" if base else f"{'-':>15}"
        say(f"{bs:>10} {med:>8.3f} {args.clips / med:>9.1f} {1e3 * med / args.clips:>8.2f} {secs.sum() / med:>10.0f} {rel}   "
            + " ".join(f"{t:.3f}" for t in ts))
    if 1 in results:
        for bs in sizes:
            same = sum(a == b for a, b in zip(results[bs], results[1]))
            nb = sum(len(r) * 2 for r in results[1])
            eq = sum(x[0] == y[0] and x[1] == y[1] for a, b in zip(results[bs], results[1]) for x, y in zip(a, b)) * 2
            say(f"# batch_size {bs}: {same} of {args.clips} records with every boundary equal to batch_size 1's ({eq} of {nb} boundaries)")
    if args.stages:
        from lyricalignment_amd.audio_frontend import log_mel_spectrogram_per_clip
        from lyricalignment_amd.utils.alignment import _labels_to_device
        from lyricalignment_amd.module.align_model import frame_plan
        order = sorted(range(args.clips), key=lambda i: len(records[i].audio))
        eng = model.engine()
        say("")
        say(f"{'clips':>5} {'longest s':>9} {'log-mel ms':>10} {'encoder ms':>10} {'head+DP ms':>10} {'sum / clip':>10}")
        with torch.no_grad():
            for bs in sizes:
                idx = order[-bs:]
                audios = [records[i].audio for i in idx]
                labels = [by_text[records[i].text] for i in idx]
                lab, n_lab, _ = _labels_to_device(labels, bs, eng.device)
                for _ in range(2):
                    t_mel, (mel, n_mel) = _event_ms(lambda: log_mel_spectrogram_per_clip(audios, device=eng.device))
                    t_enc, feats = _event_ms(lambda: eng.encode(mel))
                    T = [frame_plan(n, True)[0][2] for n in n_mel]
                    nf = torch.tensor(T, dtype=torch.int32).to(eng.device)
                    t_head, _ = _event_ms(lambda: eng.align_feats_checked(feats, bs, max(T), 1500, lab, n_lab, _lib.LA_VARIANT_CTC, n_frames=nf))
                say(f"{bs:>5} {len(audios[-1]) / 16000:>9.2f} {t_mel:>10.2f} {t_enc:>10.2f} {t_head:>10.2f} {(t_mel + t_enc + t_head) / bs:>10.2f}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
