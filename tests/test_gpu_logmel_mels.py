"""The 128-bin log-mel front end (whisper large-v3 / large-v3-turbo) on the device, from the kernel to AlignModel: la_logmel_*_n at
n_mels = 128 against the float32 restatement of the oracle's recipe (tests/logmel_reference.py, pinned on the CPU by
tests/test_host_logmel_mels.py), the same entries at n_mels = 80 against the 80-bin entries bit for bit, and a small 128-bin model --
whose conv stem has no pad channels -- through embed_audio, align and the encoder's backward against the CPU oracle.

Tolerances: 2e-4 on the log-mel (tests/test_gpu_model.py test_log_mel_matches_oracle's bound for the 80-bin kernel; the error sources --
a float32 DFT by products against a float32 FFT -- are the same), 1e-3 on encoder outputs (test_encoder_matches_oracle), seconds equal.
Largest log-mel error measured on MI355X when this was written: see DESIGN.md section 4 (log-mel)."""
import ctypes

import numpy as np
import pytest
import torch

import logmel_reference as lr

pytestmark = pytest.mark.gpu

ATOL = 2e-4


def _batch3(n):
    """test_log_mel_ragged_lengths_and_the_one_call_entry_point's batch: three levels, so the whole-tensor maximum that sets clip 0's
    floor sits in clip 1's tiles."""
    return np.stack([lr.wave(n, 4) * 1e-3, lr.wave(n, 5), lr.wave(n, 6) * 0.1])


def _tables(n_mels):
    from lyricalignment_amd.audio_frontend import _device_tables
    return _device_tables(torch.cuda.current_device(), n_mels)


def _workspace(L, n_mels, B, n):
    need = ctypes.c_size_t(0)
    assert L.la_logmel_workspace_bytes_n(n_mels, B, n, ctypes.byref(need)) == 0
    return torch.empty((need.value,), dtype=torch.uint8, device="cuda"), need.value


def _fresh_constants(n_mels, entry=None):
    """Constants in a buffer of this test's own (audio_frontend's cached ones stay untouched): entry None = la_logmel_constants_n,
    else the 80-bin la_logmel_constants."""
    from lyricalignment_amd import _lib
    L = _lib.lib()
    filt, win = _tables(n_mels)
    need = ctypes.c_size_t(0)
    assert L.la_logmel_constants_bytes_n(n_mels, ctypes.byref(need)) == 0
    c = torch.zeros((need.value,), dtype=torch.uint8, device="cuda")
    if entry is None:
        _lib.check(L.la_logmel_constants_n(n_mels, _lib.ptr(filt), _lib.ptr(win), _lib.ptr(c), need.value, _lib.stream_ptr()), "constants_n")
    else:
        _lib.check(L.la_logmel_constants(_lib.ptr(filt), _lib.ptr(win), _lib.ptr(c), need.value, _lib.stream_ptr()), "constants")
    return c


# ------------------------------------------------------------------------------------------------ 1. dense form at 128 bins
def test_log_mel_128_matches_the_restatement_at_tile_edges():
    """Lengths with both reflect pads inside one tile, a partial last tile and one frame past a tile, three levels per batch; shape,
    untouched slack behind a wider row pitch, and la_logmel_f32_n (constants built in the call) = la_logmel_f32_prepared_n bit for bit."""
    from lyricalignment_amd import _lib
    from lyricalignment_amd.audio_frontend import log_mel_spectrogram
    L = _lib.lib()
    filt, win = _tables(128)
    worst = 0.0
    for n in lr.LENGTHS:
        batch = _batch3(n)
        ours = log_mel_spectrogram(batch, n_mels=128)
        ref = lr.logmel_ref(batch, 128)
        assert tuple(ours.shape) == tuple(ref.shape) == (3, 128, n // 160) and ours.dtype == torch.float32
        err = float((ours.cpu() - ref).abs().max())
        worst = max(worst, err)
        print(f"128 bins, {n} samples x 3 levels: max |log-mel error| {err:.2e}")
        np.testing.assert_allclose(ours.cpu().numpy(), ref.numpy(), rtol=0, atol=ATOL, err_msg=str(n))
        a = torch.from_numpy(batch).cuda()
        mel = torch.full((3, 128, n // 160 + 5), 7.0, device="cuda")                   # row pitch > frames: the slack stays untouched
        ws, ws_bytes = _workspace(L, 128, 3, n)
        _lib.check(L.la_logmel_f32_n(128, _lib.ptr(a), 3, n, _lib.ptr(filt), _lib.ptr(win), _lib.ptr(mel), mel.stride(0), mel.stride(1),
                                     _lib.ptr(ws), ws_bytes, _lib.stream_ptr()), "logmel_f32_n")
        assert torch.equal(mel[:, :, : n // 160], ours) and bool((mel[:, :, n // 160:] == 7.0).all())
    pair = np.stack([lr.wave(60096, 1), lr.wave(60096, 2) * 1e-2])
    ours = log_mel_spectrogram(pair, n_mels=128).cpu()
    err = float((ours - lr.logmel_ref(pair, 128)).abs().max())
    print(f"128 bins, 60096 samples x 2: max |log-mel error| {err:.2e}; largest of this test {max(worst, err):.2e}")
    assert tuple(ours.shape) == (2, 128, 375)
    np.testing.assert_allclose(ours.numpy(), lr.logmel_ref(pair, 128).numpy(), rtol=0, atol=ATOL)
    one = log_mel_spectrogram(lr.wave(12345, 7), n_mels=128)                            # a 1-D waveform: no batch axis in the result
    assert tuple(one.shape) == (128, 77) and torch.equal(one, log_mel_spectrogram(lr.wave(12345, 7)[None], n_mels=128)[0])
    with pytest.raises(ValueError):
        log_mel_spectrogram(lr.wave(200, 1), n_mels=128)


# ------------------------------------------------------------------------------------------------ 2. the _n entries at 80 bins
def test_n_entries_at_80_bins_are_the_80_bin_entries_bit_for_bit():
    from lyricalignment_amd import _lib, ops
    L = _lib.lib()
    filt, win = _tables(80)
    c_old, c_new = _fresh_constants(80, entry="la_logmel_constants"), _fresh_constants(80)
    assert torch.equal(c_old, c_new)

    def dense(fn, n_mels_arg, a, n, consts):
        mel = torch.full((3, 80, n // 160 + 3), 7.0, device="cuda")
        ws, ws_bytes = _workspace(L, 80, 3, n)
        mid = (_lib.ptr(filt), _lib.ptr(win)) if consts is None else (_lib.ptr(consts),)
        _lib.check(fn(*n_mels_arg, _lib.ptr(a), 3, n, *mid, _lib.ptr(mel), mel.stride(0), mel.stride(1), _lib.ptr(ws), ws_bytes,
                      _lib.stream_ptr()), "logmel")
        return mel

    for n in lr.LENGTHS:
        a = torch.from_numpy(_batch3(n)).cuda()
        old = dense(L.la_logmel_f32_prepared, (), a, n, c_old)
        assert bool((old[:, :, n // 160:] == 7.0).all()) and bool(torch.isfinite(old).all())
        assert torch.equal(dense(L.la_logmel_f32_prepared_n, (80,), a, n, c_new), old), n
        assert torch.equal(dense(L.la_logmel_f32_prepared_n, (80,), a, n, c_old), old), n      # either buffer through either entry
        assert torch.equal(dense(L.la_logmel_f32, (), a, n, None), old), n
        assert torch.equal(dense(L.la_logmel_f32_n, (80,), a, n, None), old), n
    # the ragged form on the six clips of tests/test_gpu_ragged.py's log-mel test
    audios = [lr.clip(i) for i in range(6)]
    ns = [len(x) for x in audios]
    batch = np.zeros((6, max(ns)), dtype=np.float32)
    for i, x in enumerate(audios):
        batch[i, : ns[i]] = x
    a = torch.from_numpy(batch).cuda()
    nsd = torch.tensor(ns, dtype=torch.int32).cuda()
    old = torch.full((6, 80, 3000), 7.0, device="cuda")
    ws, ws_bytes = _workspace(L, 80, 6, max(ns))
    _lib.check(L.la_logmel_ragged_f32_prepared(_lib.ptr(a), _lib.ptr(nsd), 6, max(ns), _lib.ptr(c_old), _lib.ptr(old), old.stride(0), old.stride(1),
                                               3000, _lib.ptr(ws), ws_bytes, _lib.stream_ptr()), "ragged")
    new = torch.full((6, 80, 3000), 7.0, device="cuda")
    _lib.check(L.la_logmel_ragged_f32_prepared_n(80, _lib.ptr(a), _lib.ptr(nsd), 6, max(ns), _lib.ptr(c_new), _lib.ptr(new), new.stride(0),
                                                 new.stride(1), 3000, _lib.ptr(ws), ws_bytes, _lib.stream_ptr()), "ragged_n")
    assert torch.equal(new, old) and not bool((old == 7.0).any())
    assert torch.equal(ops.logmel_ragged(a, ns, c_new, 3000), old) and torch.equal(ops.logmel_ragged(a, ns, c_new, 3000, n_mels=80), old)


def test_constants_of_one_bin_count_are_refused_for_the_other():
    from lyricalignment_amd import _lib, ops
    L = _lib.lib()
    c80, c128 = _fresh_constants(80), _fresh_constants(128)
    n = 12345
    a = torch.from_numpy(_batch3(n)).cuda()
    nsd = torch.tensor([n, n - 100, n - 3000], dtype=torch.int32).cuda()
    for n_mels, wrong, right in ((128, c80, c128), (80, c128, c80)):
        other = 80 if n_mels == 128 else 128
        mel = torch.full((3, n_mels, 3000), 7.0, device="cuda")
        ws, ws_bytes = _workspace(L, n_mels, 3, n)
        tail = (_lib.ptr(ws), ws_bytes, _lib.stream_ptr())
        rc = L.la_logmel_f32_prepared_n(n_mels, _lib.ptr(a), 3, n, _lib.ptr(wrong), _lib.ptr(mel), mel.stride(0), mel.stride(1), *tail)
        assert rc == _lib.LA_EINVAL and f"built for {other} mel bins" in _lib.last_error(), _lib.last_error()
        rc = L.la_logmel_ragged_f32_prepared_n(n_mels, _lib.ptr(a), _lib.ptr(nsd), 3, n, _lib.ptr(wrong), _lib.ptr(mel), mel.stride(0),
                                               mel.stride(1), 3000, *tail)
        assert rc == _lib.LA_EINVAL and f"built for {other} mel bins" in _lib.last_error(), _lib.last_error()
        with pytest.raises(ValueError):
            ops.logmel_ragged(a, [n, n - 100, n - 3000], wrong, 3000, n_mels=n_mels)
        torch.cuda.synchronize()
        assert bool((mel == 7.0).all())                                                   # refused before any launch
        assert L.la_logmel_f32_prepared_n(n_mels, _lib.ptr(a), 3, n, _lib.ptr(right), _lib.ptr(mel), mel.stride(0), mel.stride(1), *tail) == 0
    rc = L.la_logmel_f32_prepared(_lib.ptr(a), 3, n, _lib.ptr(c128), _lib.ptr(mel), mel.stride(0), mel.stride(1), *tail)   # the 80-bin name
    assert rc == _lib.LA_EINVAL and "built for 128 mel bins" in _lib.last_error()
    # building again at the same address replaces the record
    filt, win = _tables(80)
    _lib.check(L.la_logmel_constants_n(80, _lib.ptr(filt), _lib.ptr(win), _lib.ptr(c128), c128.numel(), _lib.stream_ptr()), "constants_n")
    assert L.la_logmel_f32_prepared(_lib.ptr(a), 3, n, _lib.ptr(c128), _lib.ptr(mel), mel.stride(0), mel.stride(1), *tail) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. ragged form at 128 bins
def test_logmel_per_clip_128_is_each_clip_alone():
    """tests/test_gpu_ragged.py's six clips (lengths from 9000 to 480000 samples, levels 26 dB apart) in one call: each within 2e-4 of the
    restatement of that clip alone, bit-equal to the dense 128-bin call on it alone, exact zeros past its own frames."""
    from lyricalignment_amd.audio_frontend import log_mel_spectrogram, log_mel_spectrogram_per_clip
    audios = [lr.clip(i) for i in range(6)]
    mel, n_mel = log_mel_spectrogram_per_clip(audios, n_mels=128)
    assert tuple(mel.shape) == (6, 128, 3000) and n_mel == [n // 160 for n in lr.CLIP_SAMPLES]
    for i, a in enumerate(audios):
        want = lr.logmel_ref(a[None], 128)[0]
        err = float((mel[i, :, : n_mel[i]].cpu() - want).abs().max())
        print(f"128 bins, clip {i}: n_mel {n_mel[i]}, max |log-mel error| {err:.2e}")
        np.testing.assert_allclose(mel[i, :, : n_mel[i]].cpu().numpy(), want.numpy(), rtol=0, atol=ATOL)
        assert torch.equal(mel[i, :, : n_mel[i]], log_mel_spectrogram(a[None], n_mels=128)[0])
        assert not bool(mel[i, :, n_mel[i]:].any())
    with pytest.raises(ValueError):
        log_mel_spectrogram_per_clip([audios[0], audios[0][:200]], n_mels=128)
    with pytest.raises(ValueError):
        log_mel_spectrogram_per_clip([np.zeros(480160, np.float32)], n_mels=128)


# ------------------------------------------------------------------------------------------------ 4. a 128-bin model
D, HEADS, LAYERS, HIDDEN, VOCAB = 128, 2, 2, 64, 300


@pytest.fixture(scope="module")
def small128():
    """tests/test_gpu_model.py's _small_model with n_mels = 128 (the conv stem's 128 input channels fill the kernel's channel pad), float32;
    the head peaked as in test_fused_align_vs_oracle_and_two_step_path (boundaries decided, not tie-broken).  Oracle parameters once."""
    from lyricalignment_amd import whisper_compat as wc
    from lyricalignment_amd.module.align_model import AlignModel
    dims = wc.ModelDimensions(n_mels=128, n_audio_state=D, n_audio_head=HEADS, n_audio_layer=LAYERS, n_text_state=D, n_text_head=HEADS,
                              n_text_layer=1)
    wm = wc.build_model(dims=dims, seed=0, std=0.05)
    model = AlignModel(wm, embed_dim=D, hidden_dim=HIDDEN, output_dim=VOCAB, device="cuda", compute_dtype=torch.float32)
    wc.init_align_head(model, seed=17, fc_scale=12.0)
    model.eval()
    p = {"encoder." + k: v.detach().float().cpu() for k, v in model.whisper_model.encoder.state_dict().items()}
    p.update({"align_rnn." + k: v.detach().float().cpu() for k, v in model.align_rnn.state_dict().items()})
    assert tuple(p["encoder.conv1.weight"].shape) == (D, 128, 3) and model.engine().enc.n_mels == 128
    return dict(model=model, p=p)


def _oracle_seconds(p, batch, labels):
    """The oracle pipeline at 128 bins on one zero-padded batch (what the reference's call does): seconds per clip."""
    from oracle import alignment_oracle as ao, model_oracle as mo
    T = mo.frame_count(batch.shape[1] // 160)
    with torch.no_grad():
        mel = mo.pad_or_trim(lr.logmel_ref(batch, 128), 3000)
        logits = mo.gru_head_forward(p, mo.encoder_forward(p, mel, n_head=HEADS)[:, :T])
    return ao.perform_viterbi_ctc(logits, labels)


def test_embed_audio_with_128_mel_channels_matches_oracle(small128):
    from oracle import model_oracle as mo
    model, p = small128["model"], small128["p"]
    mel = torch.rand(2, 128, 3000, generator=torch.Generator().manual_seed(5)) * 2 - 1
    with torch.no_grad():
        ours = model.whisper_model.embed_audio(mel.cuda()).cpu()
        ref = mo.encoder_forward(p, mel, n_head=HEADS)
    assert ours.shape == ref.shape == (2, 1500, D) and ours.dtype == torch.float32
    print(f"128-channel stem: max |embed_audio error| {float((ours - ref).abs().max()):.2e}")
    np.testing.assert_allclose(ours.numpy(), ref.numpy(), rtol=0, atol=1e-3)
    with pytest.raises((AssertionError, ValueError)):                                     # an 80-bin mel handed to the 128-bin model
        model.align(mel=torch.zeros(1, 80, 3000).cuda(), labels=[[5, 6, 7]])
    with pytest.raises((AssertionError, ValueError)):
        model.whisper_model.embed_audio(torch.zeros(1, 80, 3000).cuda())


def test_align_with_a_128_bin_model_equals_the_oracle_pipeline(small128):
    """Waveform in, seconds out: one 60,096-sample clip, then a 2-clip batch of different lengths with the reference's batch semantics
    (zero-padded to the longer clip, one floor, one frame count) and per_clip=True (each clip as if alone)."""
    model, p = small128["model"], small128["p"]
    rs = np.random.RandomState(16)
    audio = lr.wave(60096, 14)
    labels = torch.from_numpy(rs.randint(2, VOCAB - 1, size=(1, 11)))
    labels[0, 4] = labels[0, 3]
    want = _oracle_seconds(p, audio[None], labels)
    assert model.align([audio], labels) == want and len(want[0]) == 11
    audios = [audio, lr.wave(60096 - 9000, 15)]
    two = torch.full((2, 11), -100, dtype=torch.long)
    two[0] = labels[0]
    two[1, :6] = torch.from_numpy(rs.randint(2, VOCAB - 1, size=6))
    batch = np.zeros((2, 60096), dtype=np.float32)
    batch[0] = audios[0]; batch[1, : len(audios[1])] = audios[1]
    assert model.align(audios, two) == _oracle_seconds(p, batch, two)
    alone = [_oracle_seconds(p, a[None], two[b: b + 1, : (11, 6)[b]])[0] for b, a in enumerate(audios)]
    assert model.align(audios, two, per_clip=True) == alone
    # a model whose dims and weights disagree about the bin count: the per-clip waveform path refuses before its log-mel is launched
    model.whisper_model.dims.n_mels = 80
    try:
        with pytest.raises(ValueError, match="mel bins"):
            model.align(audios, two, per_clip=True)
    finally:
        model.whisper_model.dims.n_mels = 128


# ------------------------------------------------------------------------------------------------ 5. training
def test_conv_stem_gradients_with_128_mel_channels_match_float64_autograd(small128):
    """conv1.weight [128, 128, 3] and conv1.bias through EncoderFunction (HIP forward and backward) against float64 torch autograd through
    the oracle's encoder.  Measure and bound are tests/test_gpu_finetune.py test_encoder_backward_matches_torch_autograd's for the 80-bin
    encoder's gradients: max |g - ref| / max |ref| < 1e-3 (its output bound, 1e-4, is kept too)."""
    from lyricalignment_amd import encoder_train as et
    from oracle import model_oracle as mo
    model, p = small128["model"], small128["p"]
    enc = model.whisper_model.encoder
    g = torch.Generator().manual_seed(5)
    mel = torch.randn(2, 128, 3000, generator=g) * 0.5
    dy = torch.randn(2, 1500, D, generator=g)
    p64 = {k: v.double().requires_grad_(k in ("encoder.conv1.weight", "encoder.conv1.bias")) for k, v in p.items() if k.startswith("encoder.")}
    y_ref = mo.encoder_forward(p64, mel.double(), HEADS)
    y_ref.backward(dy.double())
    names = et.encoder_param_names(LAYERS)
    params = [dict(enc.named_parameters())[n].detach().clone().requires_grad_(True) for n in names]
    y = et.EncoderFunction.apply(mel.cuda(), enc.positional_embedding, HEADS, *params)
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-12))
    assert rel(y.detach().cpu(), y_ref.detach()) < 1e-4
    y.backward(dy.cuda())
    for n, t in list(zip(names, params))[:2]:
        ref = p64["encoder." + n].grad
        assert t.grad.shape == ref.shape
        print(f"{n}: max |g - ref| / max |ref| = {rel(t.grad.cpu(), ref):.2e}")
        assert rel(t.grad.cpu(), ref) < 1e-3, n
