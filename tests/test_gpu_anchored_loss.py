"""la_anchored_alignment_loss (csrc/la_anchor_loss.hip) on the GPU: loss and gradient on the lattice with per-state frame windows against
the float64 torch yardstick tests/anchored_loss_reference.py (pinned to enumeration and to the closed formula by
tests/test_host_anchored_loss.py, which also asserts that the cases used here have a path and that their anchors bind), the full row
width, one pinned path against the hard-target CE / BCE, open windows against the unwindowed sweep, determinism, an infeasible clip beside
a feasible one, and the Python surface (finetune.anchored_alignment_loss, utils.alignment.anchored_alignment_loss,
FineTuner.micro_step_anchored) through a tiny random-weight model.

Tolerance on nll_b and on G = dlogits * B * T_b / scale (= d nll_b / d logits): absolute (8 + E) * T * 2**-23 with E the largest |em| the
yardstick reads.  8 * T * 2**-23 is the bound every gamma cell and log_z of the sum-product sweeps is held to
(tests/test_gpu_span_posteriors.py); E * T * 2**-23 covers the float32 emissions (T cells of relative rounding 2**-23 along a path).
Every comparison prints its measured maximum beside the bound; DESIGN.md "Alignment loss on the windowed lattice" is where they go.
"""
import math

import numpy as np
import pytest
import torch

import anchored_loss_reference as alr

pytestmark = pytest.mark.gpu


def _tol(T, E):
    return (8.0 + E) * T * 2.0 ** -23


def _pack(clips, V, T=None, Lmax=None, width=None):
    """clips: dicts with x [T_b, V+1], labels, lo, hi, skip_from -> the arguments of finetune.anchored_alignment_loss (host tensors)."""
    B = len(clips)
    T = T or max(c["x"].shape[0] for c in clips)
    Lmax = Lmax or max(1, max(len(c["labels"]) for c in clips))
    W = width or V + 1
    logits = torch.zeros((B, T, W), dtype=torch.float32)
    labels = torch.full((B, Lmax), -100, dtype=torch.long)
    lo = torch.zeros((B, 2 * Lmax + 1), dtype=torch.int32)
    hi = torch.zeros((B, 2 * Lmax + 1), dtype=torch.int32)
    skip = torch.full((B, Lmax + 1), -1, dtype=torch.int32)
    for b, c in enumerate(clips):
        logits[b, : c["x"].shape[0], : V + 1] = torch.from_numpy(c["x"])
        labels[b, : len(c["labels"])] = torch.tensor(c["labels"], dtype=torch.long)
        lo[b, : len(c["lo"])] = torch.tensor(c["lo"], dtype=torch.int32)
        hi[b, : len(c["hi"])] = torch.tensor(c["hi"], dtype=torch.int32)
        if c.get("skip_from") is not None:
            skip[b, : len(c["skip_from"])] = torch.tensor(c["skip_from"], dtype=torch.int32)
    n_frames = torch.tensor([c["x"].shape[0] for c in clips], dtype=torch.int32)
    ragged = any(c["x"].shape[0] != T for c in clips)
    return logits, labels, lo, hi, (n_frames if ragged else None), (skip if any(c.get("skip_from") is not None for c in clips) else None)


def _run(clips, V, penalty=0.0, scale=1.0, logits_dev=None, **kw):
    from lyricalignment_amd import finetune as ft
    logits, labels, lo, hi, nf, skip = _pack(clips, V, **kw)
    x = logits.cuda() if logits_dev is None else logits_dev
    loss, nll, status, d = ft.anchored_alignment_loss(x, labels, lo, hi, nf, skip, penalty, vocab_size=V, scale=scale)
    torch.cuda.synchronize()
    return loss.cpu(), nll.cpu(), status.cpu(), d.cpu()


def _second_clip():
    """The batch mate of the (40, 5, 12) case: L = 3, 33 frames."""
    if "second" not in alr._CASES:
        from lyricalignment_amd.utils.alignment import windows_from_anchors
        T, L, V = 33, 3, 12
        x = (3.0 * np.random.RandomState(333).randn(T, V + 1)).astype(np.float32)
        labels = alr.labels_for(5, L, V)
        lo, hi = windows_from_anchors(L, T, onset_anchors=alr.anchors_for(T, L, 2), hop_size_second=alr.HOP)
        alr._CASES["second"] = dict(x=x, labels=labels, lo=lo, hi=hi, skip_from=None, penalty=0.0, ref=alr.clip(x, labels, V, lo, hi))
    return alr._CASES["second"]


def _compare(what, clips, V, loss, nll, status, d, scale):
    """nll and G of every clip against its yardstick -> the measured maxima (printed)."""
    B = len(clips)
    want_loss = 0.0
    for b, c in enumerate(clips):
        ref, T = c["ref"], c["x"].shape[0]
        assert ref["feasible"] and int(status[b]) == 0, (what, b)
        tol = _tol(T, ref["E"])
        G = d[b, :T, : V + 1].double().numpy() * (B * T / scale)
        e_nll, e_g = abs(float(nll[b]) - ref["nll"]), float(np.abs(G - ref["G"]).max())
        print(f"{what} clip {b}: T={T} L={len(c['labels'])} V={V}: |nll - ref| {e_nll:.2e}, max |G - ref| {e_g:.2e}, bound {tol:.2e} (E {ref['E']:.1f})")
        assert e_nll <= tol and e_g <= tol, (what, b, e_nll, e_g, tol)
        assert not d[b, T:].any() and not d[b, :, V + 1:].any() and not d[b, :, 0].any()        # exact zeros: rows past the end, column 0
        want_loss += ref["nll"] / T / B
    assert abs(float(loss[0]) - want_loss) <= 2e-6 * abs(want_loss) + max(_tol(c["x"].shape[0], c["ref"]["E"]) / c["x"].shape[0] for c in clips)


# ------------------------------------------------------------------------------------------------ 1. against the yardstick
@pytest.mark.parametrize("T,L,V", alr.GPU_SHAPES, ids=[f"T{t}_L{l}_V{v}" for t, l, v in alr.GPU_SHAPES])
def test_loss_and_gradient_match_the_float64_yardstick(T, L, V):
    from lyricalignment_amd import _lib
    variants = (0, 1, 2) if (T, L, V) == alr.SPAN_SHAPE else (0,)
    forms = (1, 0) if 2 * L + 1 <= 64 else (1,)                   # viterbi_dpp: the two one-wave forms of the sweep
    for variant in variants:
        c = alr.gpu_case(T, L, V, variant)
        clips = [c, _second_clip()] if (T, L, V) == (40, 5, 12) else [c]
        for form in forms:
            with _lib.option("viterbi_dpp", form):
                out = _run(clips, V, c["penalty"], scale=0.25)
            _compare(f"variant {variant} dpp {form}", clips, V, *out, scale=0.25)
    if (T, L, V) == (40, 5, 12):
        # a common offset of +1e4 on the word columns 1..V-1: the emissions keep a row's maximum and log-sum apart, so nothing is lost
        base = alr.gpu_case(T, L, V)
        x = base["x"].copy()
        x[:, 1:V] += np.float32(1e4)
        c = dict(base, x=x, ref=alr.clip(x, base["labels"], V, base["lo"], base["hi"]))
        _compare("word columns + 1e4", [c], V, *_run([c], V, scale=0.25), scale=0.25)


# ------------------------------------------------------------------------------------------------ 2. the real row width
def test_full_vocabulary_row_every_column():
    """V = 21128: 21129 columns a row, 21 floats per lane of the gradient kernel.  Rows of 21129 floats start at every 16-byte phase (single
    floats at both ends of the 16-byte pieces), rows of 21132 all start on a boundary (and the columns past V stay zero); logits that do
    not share the gradient's 16-byte phase take the single-float form.  Every column is compared."""
    from lyricalignment_amd.utils.alignment import windows_from_anchors
    T, L, V = 8, 3, 21128
    x = (3.0 * np.random.RandomState(8).randn(T, V + 1)).astype(np.float32)
    labels = [20000, 20000, 7]
    lo, hi = windows_from_anchors(L, T, onset_anchors=[(1, 0.06, 0.02)], hop_size_second=alr.HOP)
    c = dict(x=x, labels=labels, lo=lo, hi=hi, skip_from=None, ref=alr.clip(x, labels, V, lo, hi))
    outs = []
    for width in (V + 1, V + 4):
        out = _run([c], V, width=width)
        _compare(f"width {width}", [c], V, *out, scale=1.0)
        outs.append(out)
    assert torch.equal(outs[0][3], outs[1][3][:, :, : V + 1]) and torch.equal(outs[0][1], outs[1][1])
    buf = torch.zeros((T * (V + 1) + 4,), dtype=torch.float32, device="cuda")
    shifted = buf[1: 1 + T * (V + 1)].view(1, T, V + 1)
    shifted.copy_(torch.from_numpy(x)[None])
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    out = _run([c], V, logits_dev=shifted)
    _compare("logits off the gradient's 16-byte phase", [c], V, *out, scale=1.0)
    assert torch.equal(out[1], outs[0][1])


# ------------------------------------------------------------------------------------------------ 3. one path: the hard-target loss
def test_pinned_windows_give_the_frame_ce_and_silence_bce_with_hard_targets():
    from lyricalignment_amd import _lib, ops
    T, L, V = 40, 5, 12
    c = alr.gpu_case(T, L, V)
    labels = c["labels"]
    S = 2 * L + 1
    bounds = [0, 3, 9, 10, 14, 20, 21, 29, 33, 34, 38, 40]       # state s holds frames bounds[s] .. bounds[s+1]-1
    lo, hi = bounds[:S], bounds[1: S + 1]
    path = [s for s in range(S) for _ in range(hi[s] - lo[s])]
    pinned = dict(x=c["x"], labels=labels, lo=lo, hi=hi, skip_from=None)
    loss, nll, status, d = _run([pinned], V)
    assert int(status[0]) == 0
    lab = torch.tensor([labels], dtype=torch.int32).cuda()
    em = ops.emissions_from_logits(torch.from_numpy(c["x"])[None].cuda(), lab, torch.tensor([L], dtype=torch.int32).cuda(), _lib.LA_VARIANT_CTC)[0].cpu().double().numpy()
    cells = [em[t, 0 if s % 2 == 0 else 1 + s // 2] for t, s in enumerate(path)]
    E = max(abs(v) for v in cells)
    print(f"one path: nll {float(nll[0]):.6f}, -sum of the device's emissions {-sum(cells):.6f}, bound {T * 2.0 ** -23 * E:.2e}")
    assert abs(float(nll[0]) + sum(cells)) <= T * 2.0 ** -23 * E
    x64 = c["x"].astype(np.float64)
    want = np.zeros((T, V + 1))
    word = x64[:, 1:V]
    sm = np.exp(word - word.max(1, keepdims=True))
    sm /= sm.sum(1, keepdims=True)
    sig = 1.0 / (1.0 + np.exp(-x64[:, V]))
    for t, s in enumerate(path):
        if s % 2:
            want[t, 1:V] = sm[t]
            want[t, labels[s // 2]] -= 1.0
            want[t, V] = sig[t]
        else:
            want[t, V] = sig[t] - 1.0
    G = d[0, :, : V + 1].double().numpy() * T
    print(f"one path: max |G - hard-target CE/BCE gradient| {np.abs(G - want).max():.2e}, bound {4 * 2.0 ** -23:.2e}")
    assert np.abs(G - want).max() <= 4 * 2.0 ** -23


# ------------------------------------------------------------------------------------------------ 4. open windows
def test_open_windows_give_the_unwindowed_log_partition_bit_for_bit():
    from lyricalignment_amd import _lib, ops
    clips = []
    for (T, L, V) in ((40, 5, 12), (100, 32, 40)):
        c = alr.gpu_case(T, L, V)
        clips.append((V, dict(x=c["x"], labels=c["labels"], lo=[0] * (2 * L + 1), hi=[T] * (2 * L + 1), skip_from=None)))
    for V, c in clips:
        loss, nll, status, d = _run([c], V)
        T, L = c["x"].shape[0], len(c["labels"])
        x = torch.from_numpy(c["x"])[None].cuda()
        lab = torch.tensor([c["labels"]], dtype=torch.int32).cuda()
        n_lab, nf = torch.tensor([L], dtype=torch.int32).cuda(), torch.tensor([T], dtype=torch.int32).cuda()
        em = ops.emissions_from_logits(x, lab, n_lab, _lib.LA_VARIANT_CTC)
        on, off, _, st = ops.viterbi_batch(em, lab, n_lab, nf)
        log_z = ops.alignment_posteriors(em, lab, n_lab, nf, on, off)[3].cpu()
        assert int(status[0]) == 0 and float(nll[0]) == -float(log_z[0]), (float(nll[0]), float(log_z[0]))
        assert float(loss[0]) == np.float32(float(nll[0]) / T)


# ------------------------------------------------------------------------------------------------ 5. determinism
def test_two_calls_agree_bit_for_bit_and_a_clip_does_not_depend_on_its_batch_mates():
    T, L, V = 40, 5, 12
    a, b = alr.gpu_case(T, L, V), _second_clip()
    s = 0.75
    first, again = _run([a, b], V, scale=s), _run([a, b], V, scale=s)
    for u, v in zip(first, again):
        assert torch.equal(u, v)
    for i, c in enumerate((a, b)):                                # alone: the same frame and label capacity, half the scale
        loss, nll, status, d = _run([c], V, scale=s / 2, T=T, Lmax=L)
        assert torch.equal(nll[0], first[1][i]) and torch.equal(d[0], first[3][i]), i
    # a class at several positions: the chain's order is fixed, so a larger repeated-class case repeats too
    big = alr.gpu_case(300, 100, 121)
    assert torch.equal(_run([big], 121)[3], _run([big], 121)[3])


# ------------------------------------------------------------------------------------------------ 6. an infeasible clip beside a feasible one
def test_infeasible_and_empty_clips_beside_a_feasible_one():
    from lyricalignment_amd import _lib
    from lyricalignment_amd.utils import alignment as ua
    T, L, V = 40, 5, 12
    ok = alr.gpu_case(T, L, V)
    dead = dict(x=ok["x"], labels=ok["labels"], lo=[1] * (2 * L + 1), hi=[T] * (2 * L + 1), skip_from=None)      # every state closed at frame 0
    loss, nll, status, d = _run([ok, dead], V)
    assert status.tolist() == [_lib.LA_OK, _lib.LA_EINFEASIBLE]
    assert math.isinf(float(nll[1])) and float(nll[1]) > 0 and not d[1].any()
    assert d[0].abs().max() > 0
    want = ok["ref"]["nll"] / T / 2                               # the sum is still divided by the batch
    assert abs(float(loss[0]) - want) <= 2e-6 * want + _tol(T, ok["ref"]["E"]) / T
    G = d[0, :, : V + 1].double().numpy() * (2 * T)
    assert np.abs(G - ok["ref"]["G"]).max() <= _tol(T, ok["ref"]["E"])
    empty = dict(x=ok["x"], labels=[], lo=[0], hi=[T], skip_from=None)
    loss3, nll3, status3, d3 = _run([ok, dead, empty], V)
    assert status3.tolist() == [_lib.LA_OK, _lib.LA_EINFEASIBLE, _lib.LA_EEMPTY] and math.isinf(float(nll3[2])) and not d3[2].any()
    assert abs(float(loss3[0]) - ok["ref"]["nll"] / T / 3) <= 2e-6 * want + _tol(T, ok["ref"]["E"]) / T
    # the autograd wrapper: "raise" names the clip, "skip" returns the feasible clip's share
    x = torch.from_numpy(np.stack([ok["x"], ok["x"]])).cuda().requires_grad_(True)
    labels = torch.tensor([ok["labels"], ok["labels"]])
    anchors = [ok["anchors"], [(0, 0.5, 0.02), (1, 0.1, 0.02)]]    # clip 1: character 1 has to start four tenths of a second before character 0 ends
    with pytest.raises(ValueError, match="clip 1"):
        ua.anchored_alignment_loss(x, labels, onset_anchors=anchors)
    got = ua.anchored_alignment_loss(x, labels, onset_anchors=anchors, on_infeasible="skip")
    assert got.requires_grad and abs(float(got) - want) <= 2e-6 * want + _tol(T, ok["ref"]["E"]) / T
    got.backward()
    assert not x.grad[1].any() and np.abs(x.grad[0].cpu().double().numpy() * (2 * T) - ok["ref"]["G"]).max() <= _tol(T, ok["ref"]["E"])
    # no constraint at all: every window is open
    free = ua.anchored_alignment_loss(x.detach(), labels)
    assert float(free) < float(got) * 2


# ------------------------------------------------------------------------------------------------ 7. through the model
def _tiny_model():
    from lyricalignment_amd import whisper_compat as wc
    from lyricalignment_amd.module.align_model import AlignModel
    dims = wc.ModelDimensions(n_audio_state=128, n_audio_head=2, n_audio_layer=1, n_text_state=128, n_text_head=2, n_text_layer=0)
    torch.manual_seed(17)
    model = AlignModel(wc.build_model(dims=dims, seed=81, std=0.05), embed_dim=128, hidden_dim=64, output_dim=41, dropout=0.0,
                       freeze_encoder=True, device="cuda").to("cuda")
    for p_ in model.whisper_model.parameters():
        p_.requires_grad_(False)
    return model


def test_micro_step_anchored_head_gradients_match_float64_autograd_and_the_plain_loop():
    """One clip with two anchors through the smallest model tests/test_gpu_finetune.py builds (width 128, one block, frozen encoder):
    the head-parameter gradients in the flat bucket after FineTuner.micro_step_anchored against float64 autograd through the oracle's
    head and the yardstick loss -- measure and tolerance of test_full_finetune_micro_step_gradients_match_torch_autograd (per parameter,
    largest difference over the largest reference entry, 2e-3) --, FineTuner.step() after it, and the autograd wrapper in a plain
    loss.backward() loop: the same .grad."""
    from oracle import model_oracle as mo
    from lyricalignment_amd import finetune as ft
    from lyricalignment_amd.utils import alignment as ua
    V = 40
    model = _tiny_model()
    sd = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}
    rs = np.random.RandomState(82)
    audios = [(rs.randn(16000) * 0.1).astype(np.float32)]
    labels = torch.tensor([[3, 7, 7, 12]])
    anchors = [[(1, 5.0, 1.0), (3, 20.0, 1.0)]]
    tuner = ft.FineTuner(model, vocab_size=V, world=1)
    loss = tuner.micro_step_anchored(audios, labels, onset_anchors=anchors, accum_grad_steps=2)
    got = tuner.grad[0].cpu().clone()
    # ---- float64: the oracle's encoder (no gradient: frozen) and head, the yardstick loss ----
    p = {}
    for k, v in sd.items():
        key = k[len("whisper_model."):] if k.startswith("whisper_model.") else k
        p[key] = v.double().requires_grad_(key.startswith("align_rnn."))
    mel = mo.pad_or_trim(mo.log_mel_spectrogram(audios[0][None]), 3000).double()
    with torch.no_grad():
        xa = mo.encoder_forward(p, mel, n_head=2)
    logits = mo.gru_head_forward(p, xa)[0]
    T = logits.shape[0]
    lab = [3, 7, 7, 12]
    lo, hi = ua.windows_from_anchors(4, T, onset_anchors=anchors[0])
    ref = -alr.log_partition(alr.emissions(logits, lab, V), lab, lo, hi) / T
    (ref / 2).backward()
    np.testing.assert_allclose(float(loss), float(ref.detach()), rtol=2e-4)
    off, worst = 0, {}
    for name, prm in model.align_rnn.named_parameters():
        g = got[off: off + prm.numel()].view(prm.shape); off += prm.numel()
        want = p["align_rnn." + name].grad
        worst[name] = float((g - want).abs().max() / want.abs().max().clamp_min(1e-12))
    print("head-parameter gradients against float64:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert off == got.numel() and not {k: v for k, v in worst.items() if v > 2e-3}, worst
    tuner.step()
    assert tuner.steps_done == 1 and not tuner.grad[0].any()
    # ---- the plain loop on a second copy of the model ----
    plain = _tiny_model()
    plain.load_state_dict(sd)
    plain.train()
    align_logit, _ = plain.frame_manual_forward(audios, get_orig_len=False)
    l2 = ua.anchored_alignment_loss(align_logit, labels, onset_anchors=anchors)
    assert l2.grad_fn is not None
    (l2 / 2).backward()
    np.testing.assert_allclose(float(l2), float(loss), rtol=1e-6)
    flat = torch.cat([prm.grad.reshape(-1) for prm in plain.align_rnn.parameters()]).cpu()
    np.testing.assert_allclose(flat.numpy(), got.numpy(), rtol=0, atol=1e-6 * float(got.abs().max()))
    # an infeasible clip raises after the backward; the plain variant has no such loss
    with pytest.raises(ValueError, match="clip 0"):
        tuner.micro_step_anchored(audios, labels, onset_anchors=[[(0, 20.0, 0.02), (1, 5.0, 0.02)]])
    for g in tuner.grad:
        assert not g.any()                                           # its rows were zero
    tuner.use_ctc_loss = False
    with pytest.raises(ValueError, match="CTC variant"):
        tuner.micro_step_anchored(audios, labels, onset_anchors=anchors)
