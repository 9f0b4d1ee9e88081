"""Batches of clips of different lengths, each aligned as if it ran alone (AlignModel.align(per_clip=True) and the layers under
it: la_logmel_ragged_f32_prepared, la_gru_layer_ragged, la_align_head_forward_ragged).

The yardstick of every number is the CPU oracle run ONE CLIP AT A TIME (oracle/model_oracle.py, oracle/alignment_oracle.py), or
torch.nn.GRU run per clip on that clip's own frames -- never this project's dense path, which appears only as the contrast in
test_per_clip_false_still_couples and as bookkeeping in the harness test.

Inputs are seeded recipes: clip i has NS[i] samples, 0.05 randn(seed i) + 0.3 sin(2 pi (180 + 40 i) t) + 0.2 sin(2 pi 3000 t (1 + 0.1 t)), and LS[i]
labels RandomState(10 + i).randint(2, 403) with one repeated neighbour.  At the Whisper-tiny dimensions with this file's model the oracle's
own boundaries of all six clips survive five draws of uniform +-1e-3 noise on the logits (both DP variants; checked on the CPU when the test
was written), so equality of seconds is a fair demand of logits that are held within 1e-3."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_gpu_parity_full import VOCAB, _build, _count_launches, _flat

pytestmark = pytest.mark.gpu

NS = [60096, 24237, 101760, 48160, 480000, 9000]
LS = [11, 5, 17, 8, 26, 3]
TS = [188, 76, 318, 150, 1500, 28]                  # round(n_mel / 2), banker's rounding (frame_plan)


def _clip(i, amp=1.0):
    n = NS[i]
    rs = np.random.RandomState(i)
    t = np.arange(n) / 16000.0
    x = rs.randn(n) * 0.05 + 0.3 * np.sin(2 * np.pi * (180 + 40 * i) * t) + 0.2 * np.sin(2 * np.pi * 3000 * t * (1 + 0.1 * t))
    return (amp * x).astype(np.float32)


def _clip_labels(i):
    lab = np.random.RandomState(10 + i).randint(2, 403, size=LS[i])
    if LS[i] > 3:
        lab[3] = lab[2]
    return torch.from_numpy(lab[None])


def _padded_labels(idx):
    out = torch.full((len(idx), max(LS[i] for i in idx)), -100, dtype=torch.long)
    for r, i in enumerate(idx):
        out[r, : LS[i]] = _clip_labels(i)[0]
    return out


def _oracle_params(model):
    p = {"encoder." + k: v.detach().float().cpu() for k, v in model.whisper_model.encoder.state_dict().items()}
    p.update({"align_rnn." + k: v.detach().float().cpu() for k, v in model.align_rnn.state_dict().items()})
    return p


def _oracle_logits(p, dims, audio):
    """The oracle on ONE clip: logits [1, T, V], T."""
    from oracle import model_oracle as mo
    mel = mo.pad_or_trim(mo.log_mel_spectrogram(audio[None]), 3000)
    T = mo.frame_count(len(audio) // 160)
    with torch.no_grad():
        return mo.gru_head_forward(p, mo.encoder_forward(p, mel, n_head=dims.n_audio_head)[:, :T]), T


@pytest.fixture(scope="module")
def tiny():
    """Whisper-tiny dimensions, float32, and the per-clip oracle's logits / seconds of the six clips (computed once)."""
    from oracle import alignment_oracle as ao
    model, dims = _build("tiny", torch.float32)
    p = _oracle_params(model)
    ref = []
    for i in range(6):
        lg, T = _oracle_logits(p, dims, _clip(i))
        assert T == TS[i]
        ref.append(dict(logits=lg, T=T, ctc=ao.perform_viterbi_ctc(lg, _clip_labels(i))[0], plain=ao.perform_viterbi(lg, _clip_labels(i))[0]))
    return dict(model=model, dims=dims, wm=model.whisper_model, ref=ref)


# ------------------------------------------------------------------------------------------------ 1. log-mel
def test_logmel_per_clip_matches_oracle_per_clip():
    """Six clips of different lengths AND levels (the per-clip maxima differ by up to 26 dB, so a shared floor would show) in one
    call: every clip against the oracle's log-mel of that clip alone, pad_or_trim'ed; atol 2e-4 (test_log_mel_matches_oracle's),
    the zeros past the clip's own frames exact."""
    from lyricalignment_amd.audio_frontend import log_mel_spectrogram_per_clip
    from oracle import model_oracle as mo
    amps = [1.0, 0.5, 2.0, 0.25, 1.5, 0.1]
    audios = [_clip(i, amps[i]) for i in range(6)]
    mel, n_mel = log_mel_spectrogram_per_clip(audios)
    assert tuple(mel.shape) == (6, 80, 3000) and n_mel == [n // 160 for n in NS]
    got = mel.cpu().numpy()
    for i, a in enumerate(audios):
        want = mo.pad_or_trim(mo.log_mel_spectrogram(a[None]), 3000)[0].numpy()
        err = float(np.abs(got[i] - want).max())
        print(f"clip {i}: n_mel {n_mel[i]}, max |log-mel error| {err:.2e}")
        np.testing.assert_allclose(got[i], want, rtol=0, atol=2e-4)
        assert not got[i][:, n_mel[i]:].any()
    with pytest.raises(ValueError):
        log_mel_spectrogram_per_clip([audios[0], audios[0][:200]])
    with pytest.raises(ValueError):
        log_mel_spectrogram_per_clip([np.zeros(480160, np.float32)])


# ------------------------------------------------------------------------------------------------ 2. recurrence
def _lengths(B, T, seed):
    rs = np.random.RandomState(seed)
    n = rs.randint(2, max(3, T), size=B)
    n[0] = 1
    n[min(1, B - 1)] = T                               # the launch's maximum is present
    if B > 17:
        n[16], n[17] = T, 1                            # ... and both extremes in the second 16-clip group
    return [int(v) for v in n]


@pytest.mark.parametrize("B,T,H,dtype,handoff", [
    (3, 37, 64, torch.float32, 0),                     # gru_kernel<float>: the v_fma form (<= 4 clips)
    (20, 37, 128, torch.float32, 0),                   # gru_train_x2_kernel without gate stores (option x2_inference, > 4 clips)
    (20, 37, 128, torch.float32, 1),                   # gru_kernel<float>: the float32-MFMA form
    (3, 37, 64, torch.bfloat16, 0), (3, 37, 64, torch.float16, 0),          # 16-bit counter form, 4-wave workgroups
    (3, 37, 384, torch.bfloat16, 0), (3, 37, 384, torch.float16, 0),        # ... 8-wave workgroups
    (20, 37, 128, torch.bfloat16, 0), (20, 37, 128, torch.float16, 0),      # granule form
    (20, 29, 384, torch.bfloat16, 0), (20, 29, 384, torch.float16, 0),
    (40, 23, 384, torch.bfloat16, 0), (40, 23, 384, torch.float16, 0),      # three 16-clip groups
    (20, 37, 128, torch.bfloat16, 1),                  # counter form over two groups
])
def test_gru_layer_ragged_matches_torch_gru_per_clip(B, T, H, dtype, handoff):
    """ops.gru_layer(..., n_frames=) against torch.nn.GRU run PER CLIP on that clip's first T_b frames; rows t < T_b only, with
    test_gru_layer's tolerances.  The input projections of the frames past a clip's end are NaN: the kernels must select, not mask."""
    from lyricalignment_amd import _lib, ops
    I = 48
    gru = torch.nn.GRU(I, H, num_layers=1, batch_first=True, bidirectional=True)
    g = torch.Generator().manual_seed(140 + T + B)
    nfr = _lengths(B, T, 7 + B)
    with torch.no_grad():
        for prm in gru.parameters():
            prm.copy_((torch.rand(prm.shape, generator=g) * 2 - 1) * (1.0 / H ** 0.5))
        w_hh = torch.stack([gru.weight_hh_l0, gru.weight_hh_l0_reverse])
        if dtype != torch.float32:
            gru.weight_hh_l0.copy_(w_hh[0].to(dtype).float()); gru.weight_hh_l0_reverse.copy_(w_hh[1].to(dtype).float())
        x = torch.randn(B, T, I, generator=g)
        refs = [gru(x[b: b + 1, : nfr[b]])[0][0] for b in range(B)]
        gi = torch.stack([x @ gru.weight_ih_l0.T + gru.bias_ih_l0, x @ gru.weight_ih_l0_reverse.T + gru.bias_ih_l0_reverse], dim=2)
        for b in range(B):
            gi[b, nfr[b]:] = float("nan")
        b_hh = torch.stack([gru.bias_hh_l0, gru.bias_hh_l0_reverse])
    nf = torch.tensor(nfr, dtype=torch.int32).cuda()
    with _lib.option("gru_handoff", handoff):
        out, out_mish, flag = ops.gru_layer(gi.contiguous().cuda(), w_hh.to(dtype).contiguous().cuda(), b_hh.contiguous().cuda(), want_mish=True,
                                            n_frames=nf)
        torch.cuda.synchronize()
    assert int(flag.item()) == 0, "bounded wait in the persistent GRU kernel timed out"
    tol = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}[dtype]
    o, m = out.float().cpu(), out_mish.float().cpu()
    worst = 0.0
    for b in range(B):
        worst = max(worst, float((o[b, : nfr[b]] - refs[b]).abs().max()))
        np.testing.assert_allclose(o[b, : nfr[b]].numpy(), refs[b].numpy(), rtol=0, atol=tol, err_msg=f"clip {b} of {nfr[b]} frames")
        np.testing.assert_allclose(m[b, : nfr[b]].numpy(), torch.nn.functional.mish(refs[b]).numpy(), rtol=0, atol=tol)
    print(f"B={B} T={T} H={H} {dtype} handoff={handoff}: lengths {nfr[:4]}.., max |h error| {worst:.2e} (tol {tol:.0e})")
    with pytest.raises(ValueError):
        ops.gru_layer(gi.contiguous().cuda(), w_hh.to(dtype).contiguous().cuda(), b_hh.contiguous().cuda(), n_frames=nf[:-1])


# ------------------------------------------------------------------------------------------------ 3. end to end, float32
def _check_against_oracle(tiny, model, idx, head_logits=True):
    """Clips idx (indices into the six; repeats allowed) through the per-clip mode in ONE batch; everything against the per-clip oracle."""
    from lyricalignment_amd.utils import alignment as ua
    ref = tiny["ref"]
    audios, labels = [_clip(i) for i in idx], _padded_labels(idx)
    with torch.no_grad():
        lg = model.frame_logits_per_clip(audios)
        ctc = model.align(audios, labels, use_ctc=True, per_clip=True)
        plain = model.align(audios, labels, use_ctc=False, per_clip=True)
        Tmax = max(t.shape[0] for t in lg)
        pad = torch.zeros((len(idx), Tmax, VOCAB), dtype=torch.float32, device=lg[0].device)
        for r, t in enumerate(lg):
            pad[r, : t.shape[0]] = t
        two_ctc = ua.perform_viterbi_ctc(pad, labels, n_frames=[t.shape[0] for t in lg])
        two_plain = ua.perform_viterbi(pad, labels, n_frames=[t.shape[0] for t in lg])
    for r, i in enumerate(idx):
        assert tuple(lg[r].shape) == (TS[i], VOCAB)
        err = float((lg[r].cpu() - ref[i]["logits"][0]).abs().max())
        print(f"row {r} = clip {i}: T {TS[i]}, max |logit error| {err:.2e}")
        np.testing.assert_allclose(lg[r].cpu().numpy(), ref[i]["logits"][0].numpy(), rtol=0, atol=1e-3)
    for r, i in enumerate(idx):
        assert ctc[r] == ref[i]["ctc"], (r, i)
        assert plain[r] == ref[i]["plain"], (r, i)
        assert two_ctc[r] == ref[i]["ctc"] and two_plain[r] == ref[i]["plain"], (r, i)


@pytest.mark.parametrize("route,copies", [("f32_mfma", 1), ("f16x2", 3)])
def test_tiny_dims_per_clip_equals_oracle_per_clip(tiny, route, copies):
    """Whisper-tiny dimensions, float32, the six clips (11, 5, 17, 8, 26, 3 labels) in one batch -- and the set three times = 18 clips,
    from which the encoder's Linears run on the f16 matrix pipe: logits of every row within 1e-3 of the per-clip oracle (a stage left
    coupled to the batch is off by 0.3 or more), seconds == the per-clip oracle's for both DP variants, fused and two-step."""
    model = tiny["model"]
    idx = list(range(6)) * copies
    with torch.no_grad(), _count_launches("gemm_f16x2") as x2:
        model.frame_logits_per_clip([_clip(i) for i in idx])
    # 4 blocks x 4 Linears of the encoder run as f16x2 products only on the second route; the head adds at most its 2 projections + output Linear
    print(f"{route}: {x2.n} f16x2 GEMM launches in one frame_logits_per_clip call")
    assert (x2.n >= 16) if route == "f16x2" else (x2.n < 16), x2.n
    _check_against_oracle(tiny, model, idx)


def test_tiny_dims_per_clip_with_a_tail_slice_of_the_head(tiny):
    """Seven DISTINCT-length rows with the head sliced 4 + 3 (option head_clip_cap): every slice must get its own part of the lengths."""
    from lyricalignment_amd import _lib
    with _lib.option("head_clip_cap", 4):
        _check_against_oracle(tiny, tiny["model"], [0, 1, 2, 3, 4, 5, 1])


def test_zero_frame_clip_does_not_disturb_its_batch(tiny):
    """A clip of 201 samples has one mel frame and round(1 / 2) = 0 output frames: it gets the DP's status for zero frames (LA_EINVAL, what
    la_viterbi_batch reports for n_frames = 0) and its batch mates keep the per-clip oracle's result."""
    from lyricalignment_amd import _lib
    model, ref = tiny["model"], tiny["ref"]
    audios = [_clip(1), _clip(0)[:201], _clip(5)]
    labels = torch.full((3, 5), -100, dtype=torch.long)
    labels[0, :5] = _clip_labels(1)[0]; labels[1, :2] = torch.tensor([7, 9]); labels[2, :3] = _clip_labels(5)[0]
    with torch.no_grad():
        on, off, score, status = model.align(audios, labels, per_clip=True, return_frames=True)
    assert status.tolist() == [0, _lib.LA_EINVAL, 0]
    hop = 0.02
    for r, i in ((0, 1), (2, 5)):
        got = [[float(int(a)) * hop, float(int(b)) * hop] for a, b in zip(on[r, : LS[i]].tolist(), off[r, : LS[i]].tolist())]
        assert got == ref[i]["ctc"]


def test_per_clip_rejects_what_it_does_not_define(tiny):
    model = tiny["model"]
    with pytest.raises(ValueError):
        model.align([np.zeros(480160, np.float32)], torch.tensor([[3, 4]]), per_clip=True)             # 3001 mel frames
    with pytest.raises(ValueError):
        model.align(None, torch.tensor([[3, 4]]), mel=torch.zeros(1, 80, 3000), per_clip=True)
    with pytest.raises(ValueError):
        model.align([_clip(5)], torch.tensor([[3, 4]]), get_orig_len=False, per_clip=True)


# ------------------------------------------------------------------------------------------------ 4. the default still couples
def test_per_clip_false_still_couples(tiny):
    """The five short clips through today's call (per_clip=False, the reference's batch semantics): every clip but the longest differs
    from its per-clip result, the longest equals it -- the flag is wired and the default has not moved."""
    model, ref = tiny["model"], tiny["ref"]
    idx = [0, 1, 2, 3, 5]
    audios, labels = [_clip(i) for i in idx], _padded_labels(idx)
    with torch.no_grad():
        dense = model.align(audios, labels, use_ctc=True)
        per = model.align(audios, labels, use_ctc=True, per_clip=True)
    for r, i in enumerate(idx):
        assert per[r] == ref[i]["ctc"]
        n_diff = int((_flat([dense[r]]) != _flat([per[r]])).sum())
        print(f"clip {i}: coupled batch vs alone: {n_diff} of {2 * LS[i]} boundaries differ")
        if i == 2:
            assert dense[r] == per[r]
        else:
            assert n_diff > 0, i


# ------------------------------------------------------------------------------------------------ 5. confidence
def test_per_clip_confidence_against_the_posterior_reference(tiny):
    """align(per_clip=True, return_confidence=True, return_frames=True) against tests/posterior_reference.py evaluated per clip on
    the first T_b rows of the emissions that call consumed, at that module's derived tolerance 8 * T_b * 2**-23."""
    import posterior_reference as pr
    from lyricalignment_amd import _lib
    from lyricalignment_amd.utils import alignment as ua
    model = tiny["model"]
    idx = list(range(6))
    audios, labels = [_clip(i) for i in idx], _padded_labels(idx)
    with torch.no_grad():
        on, off, score, status, occ, onp, offp, log_z = model.align(audios, labels, per_clip=True, return_confidence=True, return_frames=True,
                                                                    boundary_window=2)
        seconds, scores = model.align(audios, labels, per_clip=True, return_confidence=True)
        # the emissions of the same launch sequence (deterministic kernels: the same bits the call above consumed)
        eng = model.engine()
        feats, B, Tmax, nf, T = model._features_per_clip(audios)
        lab_dev, n_lab, lists = ua._labels_to_device(labels, B, eng.device)
        on2, off2, score2, status2, em = eng.align_feats_checked(feats, B, Tmax, 1500, lab_dev, n_lab, _lib.LA_VARIANT_CTC, want_emissions=True, n_frames=nf)
    assert T == TS and status.tolist() == [0] * 6
    assert torch.equal(on, on2) and torch.equal(off, off2) and torch.equal(score, score2)
    em = em.cpu().numpy()
    for b in idx:
        L, Tb = LS[b], TS[b]
        tol = 8 * Tb * 2.0 ** -23
        lab = lists[b]
        gamma, entry, exit_, lz = pr.posteriors(em[b, :Tb, : L + 1], lab)
        o_r, on_r, off_r = pr.scores(gamma, entry, exit_, on[b, :L].tolist(), off[b, :L].tolist(), 2)
        worst = dict(occupancy=float(np.abs(occ[b, :L].cpu().numpy() - o_r).max()), onset=float(np.abs(onp[b, :L].cpu().numpy() - on_r).max()),
                     offset=float(np.abs(offp[b, :L].cpu().numpy() - off_r).max()), log_z=abs(float(log_z[b]) - float(lz)))
        print(f"clip {b}: T_b={Tb} L={L} tol={tol:.2e}: " + json.dumps({k: float(f"{v:.2e}") for k, v in worst.items()}))
        for k, v in worst.items():
            assert v <= tol, (b, k, v, tol)
        assert scores[b]["occupancy"] == [float(v) for v in occ[b, :L].cpu().numpy()]
        assert seconds[b] == tiny["ref"][b]["ctc"]


# ------------------------------------------------------------------------------------------------ 6. 16-bit modes
@pytest.mark.parametrize("dtype,em_mean_tol,em_max_tol", [(torch.bfloat16, 0.06, 0.35), (torch.float16, 0.01, 0.06)])
def test_per_clip_16bit_emission_error(tiny, dtype, em_mean_tol, em_max_tol):
    """The throughput modes on the six clips in one batch: CTC emissions of rows t < T_b against the per-clip float32 oracle within the
    bounds test_medium_24_blocks_16bit_emission_error_and_boundary_match uses (set there at 24 blocks); the share of equal boundaries is
    printed, not asserted."""
    from lyricalignment_amd import _lib
    from lyricalignment_amd.utils import alignment as ua
    from oracle import model_oracle as mo
    model, _ = _build("tiny", dtype, tiny["wm"])
    idx = list(range(6))
    audios, labels = [_clip(i) for i in idx], _padded_labels(idx)
    with torch.no_grad():
        got = model.align(audios, labels, use_ctc=True, per_clip=True)
        eng = model.engine()
        feats, B, Tmax, nf, T = model._features_per_clip(audios)
        lab_dev, n_lab, lists = ua._labels_to_device(labels, B, eng.device)
        em = eng.emissions(feats, B, Tmax, 1500, lab_dev, n_lab, _lib.LA_VARIANT_CTC, n_frames=nf).cpu()
        eng.check_gru()
    errs = []
    for b in idx:
        L, Tb = LS[b], TS[b]
        lp, ls = mo.emission_prep_ctc(tiny["ref"][b]["logits"])
        col = torch.tensor(lists[b]) - 1
        e = torch.cat([(em[b, :Tb, 1: 1 + L] - lp[0][:, col]).abs().flatten(), (em[b, :Tb, 0] - ls[0, :, 0]).abs()])
        exact = float(np.mean(_flat([got[b]]) == _flat([tiny["ref"][b]["ctc"]])))
        print(f"{dtype} clip {b}: emission error mean {float(e.mean()):.4f} max {float(e.max()):.4f}; boundaries exact {exact:.3f}")
        errs.append(e)
        assert float(e.mean()) < em_mean_tol and float(e.max()) < em_max_tol, b
    allerr = torch.cat(errs)
    print(f"{dtype} all clips: emission error mean {float(allerr.mean()):.4f} max {float(allerr.max()):.4f}")


# ------------------------------------------------------------------------------------------------ 7. op-by-op sequence in a fresh process
_CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_gpu_ragged as tr
from lyricalignment_amd import engine
assert engine.ENGINE_PY == {want_py}
dtype = getattr(torch, {dtype!r})
model, _ = tr._build("tiny", dtype)
idx = list(range(6))
with torch.no_grad():
    res = model.align([tr._clip(i) for i in idx], tr._padded_labels(idx), per_clip=True, return_frames=True)
np.savez({out!r}, onset=res[0].cpu().numpy(), offset=res[1].cpu().numpy(), score=res[2].cpu().numpy(), status=res[3].cpu().numpy())
print("CHILD_OK")
'''


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_engine_py_sequence_equals_the_c_call_bit_for_bit(dtype, tmp_path):
    """LA_ENGINE_PY=1 (the op-by-op Python sequence) against the one-C-call path, each in a fresh process (the switch is read at import): frames,
    scores and status of the six clips equal bit for bit."""
    runs = {}
    for name, env_py in (("c", "0"), ("py", "1")):
        out = str(tmp_path / f"{name}.npz")
        env = dict(os.environ, LA_ENGINE_PY=env_py)
        script = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), want_py=env_py == "1", dtype=dtype, out=out)
        r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
        runs[name] = np.load(out)
    assert runs["c"]["status"].tolist() == [0] * 6
    for k in ("onset", "offset", "status"):
        assert np.array_equal(runs["c"][k], runs["py"][k]), k
    assert runs["c"]["score"].tobytes() == runs["py"]["score"].tobytes()


# ------------------------------------------------------------------------------------------------ 8. harness
class _Rec:
    def __init__(self, audio, text):
        self.audio, self.text = audio, text


def test_align_records_batched_returns_the_per_clip_oracle_in_the_callers_order(tiny):
    """harness.align_records(batch_size=4) on records built from the six clips (float32): onsets / offsets of the per-clip oracle with the
    right characters in the caller's order; batch_size=1 (one record per call, the path as it was) gives the same."""
    from lyricalignment_amd.harness import PinyinClassLUT, align_records
    model, ref = tiny["model"], tiny["ref"]
    lut = PinyinClassLUT([str(i) for i in range(VOCAB)], {str(i): i for i in range(VOCAB)})           # token id -> the same class id
    texts = ["".join(chr(0x4E00 + 37 * i + j) for j in range(LS[i])) for i in range(6)]
    ids = {texts[i]: [int(v) for v in _clip_labels(i)[0]] for i in range(6)}
    records = [_Rec(_clip(i), texts[i]) for i in range(6)]
    want = [[[ref[i]["ctc"][j][0], ref[i]["ctc"][j][1], texts[i][j]] for j in range(LS[i])] for i in range(6)]
    got4 = align_records(model, records, lut, lambda t: ids[t], use_ctc_loss=True, batch_size=4)
    got1 = align_records(model, records, lut, lambda t: ids[t], use_ctc_loss=True, batch_size=1)
    assert got4 == want
    assert got1 == want
    conf = align_records(model, records, lut, lambda t: ids[t], use_ctc_loss=True, with_confidence=True, batch_size=4)
    assert [[e[:3] for e in r] for r in conf] == want and all(0.0 <= e[3] <= 1.0 + 1e-3 for r in conf for e in r)
