"""Option x2_small: float32 inference on the f16 matrix pipe at every batch size (include/lyricalign.h la_gemm_f16x2_small, la_model.cpp
x2_gemm, engine.py _x2_gemm).  The 128 x 128 f16x2 kernel against float64 and the float32 kernel, bit for bit against the 256 x 256 one
where both run; then the model-level routes at 1-3 clips against the oracle, the option-off bits, and C against the op-by-op sequence."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VOCAB = 21129


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _wave(n, seed=0):
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    f = 220 * (1 + 0.3 * seed)
    return (rs.randn(n) * 0.05 + 0.3 * np.sin(2 * np.pi * f * t) + 0.2 * np.sin(2 * np.pi * 3000 * t * (1 + 0.1 * t))).astype(np.float32)


class _count_launches:
    """Launches of one kernel family (la_timer_*, exact name) inside the block."""

    def __init__(self, family):
        self.family, self.n = family, 0

    def __enter__(self):
        from lyricalignment_amd import _lib
        L = _lib.lib()
        L.la_timer_reset(); L.la_timer_sample(1000003); L.la_timer_enable(self.family.encode())
        return self

    def __exit__(self, *exc):
        from lyricalignment_amd import _lib
        L = _lib.lib()
        torch.cuda.synchronize()
        L.la_timer_disable()
        ms, timed, work, seen = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_double(0), ctypes.c_int64(0)
        L.la_timer_read_work(ctypes.byref(ms), ctypes.byref(timed), ctypes.byref(work), ctypes.byref(seen))
        self.n = int(seen.value)
        L.la_timer_reset(); L.la_timer_sample(1)
        return False


# ---------------------------------------------------------------------------------------------------------------------- kernel
EPILOGUES = ["none", "bias", "bias_gelu", "bias_residual", "gelu_grad"]


def _products(M, N, K, epi, seed):
    """(f16x2 small-kernel result, float32-kernel result, float64 reference) of one product with epilogue `epi`."""
    from lyricalignment_amd import f32x2, ops
    a, w = _rand(M, K, seed=seed), _rand(N, K, seed=seed + 1, scale=K ** -0.5)
    bias, res = _rand(N, seed=seed + 2), _rand(M, N, seed=seed + 3)
    ad, wd = a.cuda(), w.cuda()
    kw = {}
    if epi in ("bias", "bias_gelu", "bias_residual"):
        kw["bias"] = bias.cuda()
    if epi == "bias_gelu":
        kw["gelu"] = True
    if epi == "bias_residual":
        kw["residual"] = res.cuda()
    A, W = f32x2.split(ad, K), f32x2.split(wd, K)
    if epi == "gelu_grad":
        got = f32x2.gemm_small(A, W, gelu_grad_of=res.cuda()).cpu()
        u = res.double()
        gp = 0.5 * (1 + torch.erf(u / 2 ** 0.5)) + u * torch.exp(-0.5 * u * u) / (2 * np.pi) ** 0.5
        ref = (a.double() @ w.double().t()) * gp
        nat = (ops.gemm(ad, wd).cpu().double() * gp).float()
    else:
        got = f32x2.gemm_small(A, W, **kw).cpu()
        nat = ops.gemm(ad, wd, **kw).cpu()
        ref = a.double() @ w.double().t()
        if "bias" in kw:
            ref = ref + bias.double()
        if epi == "bias_gelu":
            ref = torch.nn.functional.gelu(ref)
        if epi == "bias_residual":
            ref = ref + res.double()
    return got, nat, ref


@pytest.mark.parametrize("M,N,K", [(1500, 3072, 1024), (1500, 1024, 1024), (1500, 4096, 1024), (1500, 1024, 4096), (1, 1024, 1024),
                                   (127, 1000, 1024), (300, 1096, 384), (1500, 2304, 1024)])
def test_small_kernel_is_at_least_as_accurate_as_the_float32_kernel(M, N, K):
    """la_gemm_f16x2_small on the batch-1 encoder shapes, ragged M and the GRU input projection: max |err| / max |ref| against float64 no
    larger than float32 la_gemm's on the same operands (bias epilogue, default split-K slots)."""
    got, nat, ref = _products(M, N, K, "bias", seed=M + N + K)
    e_x2 = float((got.double() - ref).abs().max() / ref.abs().max())
    e_f32 = float((nat.double() - ref).abs().max() / ref.abs().max())
    print(f"f16x2 small M={M} N={N} K={K}: {e_x2:.2e} vs float32 kernel {e_f32:.2e}")
    assert e_x2 <= max(e_f32, 4e-7) and e_x2 < 2e-6


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("M,N,K", [(1500, 1024, 1024), (127, 200, 96)])
def test_small_kernel_epilogues(M, N, K, epi):
    """Every epilogue flag (none, BIAS, BIAS | GELU, BIAS | RESIDUAL, RESIDUAL | RES_GELU_GRAD), with and without split-K slots (K = 96:
    one slot, an odd number of 32-wide sub-stages)."""
    got, nat, ref = _products(M, N, K, epi, seed=7)
    e_x2 = float((got.double() - ref).abs().max() / ref.abs().max())
    e_f32 = float((nat.double() - ref).abs().max() / ref.abs().max())
    print(f"f16x2 small {epi} M={M} N={N} K={K}: {e_x2:.2e} vs float32 kernel {e_f32:.2e}")
    assert e_x2 <= max(1.5 * e_f32, 4e-7) and e_x2 < 2e-6


@pytest.mark.parametrize("epi", ["bias_residual", "bias_gelu", "gelu_grad"])
def test_small_kernel_is_bit_identical_to_the_256_kernel(epi):
    """slots = 1 on a shape both kernels take: the same f16 MFMA sequence per output element and the same epilogue arithmetic."""
    from lyricalignment_amd import f32x2
    M, N, K = 12288, 1024, 1024
    assert f32x2.slots_for(M, N) == 1
    a, w = _rand(M, K, seed=31).cuda(), _rand(N, K, seed=32, scale=K ** -0.5).cuda()
    bias, res = _rand(N, seed=33).cuda(), _rand(M, N, seed=34).cuda()
    A, W = f32x2.split(a, K), f32x2.split(w, K)
    kw = {"bias_residual": dict(bias=bias, residual=res), "bias_gelu": dict(bias=bias, gelu=True), "gelu_grad": dict(gelu_grad_of=res)}[epi]
    big = f32x2.gemm(A, W, **kw)
    with _count_launches("gemm_f16x2_small") as c:
        small = f32x2.gemm_small(A, W, slots=1, **kw)
    assert c.n == 1
    assert torch.equal(big, small)


def test_small_kernel_split_k_is_deterministic():
    from lyricalignment_amd import f32x2
    M, N, K = 1500, 1024, 1024
    a, w = _rand(M, K, seed=41).cuda(), _rand(N, K, seed=42, scale=K ** -0.5).cuda()
    bias, res = _rand(N, seed=43).cuda(), _rand(M, N, seed=44).cuda()
    A, W = f32x2.split(a, K), f32x2.split(w, K)
    one = f32x2.gemm_small(A, W, bias=bias, residual=res, slots=4)
    two = f32x2.gemm_small(A, W, bias=bias, residual=res, slots=4)
    assert torch.equal(one, two)
    assert f32x2.slots_small(M, N, K) == 4 and torch.equal(one, f32x2.gemm_small(A, W, bias=bias, residual=res))
    flat = f32x2.gemm_small(A, W, bias=bias, residual=res, slots=1)
    assert float((one - flat).abs().max()) < 1e-5 * float(flat.abs().max())


def test_small_kernel_domain():
    from lyricalignment_amd import f32x2
    a, w = _rand(64, 48, seed=1).cuda(), _rand(64, 48, seed=2).cuda()
    with pytest.raises(NotImplementedError):
        f32x2.gemm_small(f32x2.split(a, 48), f32x2.split(w, 48))                        # K not a multiple of 32
    A, W = f32x2.split(a, 256), f32x2.split(w, 256)
    with pytest.raises(NotImplementedError):
        f32x2.gemm_small(A, W, slots=3)                                                 # 256 / 3
    with pytest.raises(NotImplementedError):
        f32x2.gemm_small(A, W, slots=16)                                                # 16 of K per slot
    with pytest.raises(ValueError):
        f32x2.gemm_small(A, f32x2.split(w, 128))
    with pytest.raises(NotImplementedError):
        f32x2.gemm(A, W)                                                                # (the 256 x 256 entry keeps its domain)


# ---------------------------------------------------------------------------------------------------------------------- model
def _head_init(model, hidden, fc_scale, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.align_rnn.named_parameters():
            s = fc_scale if n.startswith("fc.weight") else 1.5
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (s / hidden ** 0.5))


def _build(name, wm, fc_scale=12.0):
    from lyricalignment_amd import whisper_compat as wc
    from lyricalignment_amd.module.align_model import AlignModel
    dims = wc.dims_for(name)
    model = AlignModel(wm, embed_dim=dims.n_audio_state, hidden_dim=384, output_dim=VOCAB, device="cuda", compute_dtype=torch.float32).eval()
    _head_init(model, 384, fc_scale, 7)
    return model, dims


def _labels(B, L, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(2, 403, size=(B, L)))


def _oracle(model, dims, audios, labels):
    """The oracle on the whole batch (the log-mel clamps at the batch maximum): (logits, CTC seconds, plain seconds)."""
    from oracle import alignment_oracle as ao, model_oracle as mo
    p = {"encoder." + k: v.detach().float().cpu() for k, v in model.whisper_model.encoder.state_dict().items()}
    p.update({"align_rnn." + k: v.detach().float().cpu() for k, v in model.align_rnn.state_dict().items()})
    batch = np.stack(audios)
    mel = mo.pad_or_trim(mo.log_mel_spectrogram(batch), 3000)
    T = mo.frame_count(batch.shape[1] // 160)
    with torch.no_grad():
        logits = mo.gru_head_forward(p, mo.encoder_forward(p, mel, n_head=dims.n_audio_head)[:, :T])
    return logits, ao.perform_viterbi_ctc(logits, labels), ao.perform_viterbi(logits, labels)


def _run(model, audios, labels):
    from lyricalignment_amd.utils import alignment as ua
    with torch.no_grad():
        lg, _ = model.frame_manual_forward(audios)
        with _count_launches("gemm_f16x2_small") as c:
            ctc = model.align(audios, labels, use_ctc=True)
        plain = model.align(audios, labels, use_ctc=False)
        two = ua.perform_viterbi_ctc(lg, labels)
    return lg.cpu(), ctc, plain, two, c.n


@pytest.fixture(scope="module")
def medium():
    """Whisper-medium random-init weights, 30 s clips, and the B = 1 result with option x2_small as the process started (0)."""
    from lyricalignment_amd import _lib, whisper_compat as wc
    assert _lib.get_option("x2_small") == 0
    wm = wc.build_model("medium", seed=3)
    model, dims = _build("medium", wm)
    audios = [_wave(480000, s) for s in (5, 6, 7)]
    labels = _labels(3, 26, 8)
    before = _run(model, audios[:1], labels[:1])
    return dict(model=model, dims=dims, audios=audios, labels=labels, before=before)


@pytest.mark.parametrize("B", [1, 3])
def test_medium_full_depth_small_batch_on_the_f16_pipe_equals_oracle(medium, B):
    """Whisper-medium, 24 blocks, float32, option x2_small = 1, one clip and three different clips: logits within 1e-3 of the oracle,
    align() seconds (CTC and plain) and the two-step route's equal to the oracle's; >= 4 x 24 small-kernel launches per call."""
    from lyricalignment_amd import _lib
    model, dims = medium["model"], medium["dims"]
    audios, labels = medium["audios"][:B], medium["labels"][:B]
    ref_logits, want_ctc, want_plain = _oracle(model, dims, audios, labels)
    with _lib.option("x2_small", 1):
        lg, ctc, plain, two, n = _run(model, audios, labels)
        with torch.no_grad(), _count_launches("gemm_f16x2") as big:
            model.align(audios, labels, use_ctc=True)
    err = float((lg - ref_logits).abs().max())
    print(f"medium B={B} x2_small: logits max |err| vs oracle {err:.2e}, per align(): {n} gemm_f16x2_small + {big.n} gemm_f16x2 launches")
    # every encoder Linear on an f16x2 kernel; at one clip all of them on the small one, at three the QKV and MLP-up products (>= 192 tiles of
    # 256 x 256 at 4500 rows) on the 256 x 256 kernel
    assert n + big.n >= 4 * 24 and n >= (4 if B == 1 else 2) * 24, (n, big.n)
    assert err < 1e-3
    assert ctc == want_ctc and plain == want_plain and two == want_ctc


def test_option_off_launches_nothing_new_and_keeps_the_bits(medium):
    """x2_small back at 0 after it was on: no small-kernel launch, and the bits of the call made before the option was first switched on."""
    from lyricalignment_amd import _lib
    model = medium["model"]
    audios, labels = medium["audios"][:1], medium["labels"][:1]
    with _lib.option("x2_small", 1):
        _run(model, audios, labels)
    assert _lib.get_option("x2_small") == 0
    lg, ctc, plain, two, n = _run(model, audios, labels)
    lg0, ctc0, plain0, two0, n0 = medium["before"]
    assert n == 0 and n0 == 0
    assert torch.equal(lg, lg0) and ctc == ctc0 and plain == plain0 and two == two0


def test_c_entry_points_and_python_sequence_are_bit_identical_at_one_clip(medium):
    """la_encoder_forward / la_align_head_forward against engine.py's op-by-op route (LA_ENGINE_PY) at B = 1 with x2_small = 1."""
    from lyricalignment_amd import _lib, engine as eng_mod
    from lyricalignment_amd.utils import alignment as ua
    model = medium["model"]
    audios, labels = medium["audios"][:1], medium["labels"][:1]
    res = {}
    old = eng_mod.ENGINE_PY
    try:
        with _lib.option("x2_small", 1), torch.no_grad():
            for py in (False, True):
                eng_mod.ENGINE_PY = py
                model._engine = None
                eng = model.engine()
                mel = model._mel_of(audios).cuda()
                with _count_launches("gemm_f16x2_small") as c:
                    enc = eng.encode(mel, out_dtype=torch.float32).clone()
                feats, B, T, stride = model._features(mel, True)
                lab_dev, n_lab, _ = ua._labels_to_device(labels, B, eng.device)
                with _count_launches("gemm_f16x2_small") as h:
                    out = eng.align_feats(feats, B, T, stride, lab_dev, n_lab, _lib.LA_VARIANT_CTC)
                res[py] = (enc.cpu(), [t.cpu() for t in out], c.n, h.n)
    finally:
        eng_mod.ENGINE_PY = old
        model._engine = None
    assert res[False][2] >= 4 * 24 and res[True][2] >= 4 * 24 and res[False][3] >= 2 and res[True][3] >= 2, (res[False][2:], res[True][2:])
    assert torch.equal(res[False][0], res[True][0])
    for x, y in zip(res[False][1], res[True][1]):
        assert torch.equal(x, y)


def test_tiny_full_depth_two_clips_equal_oracle():
    """Whisper-tiny dims (d = 384, 4 blocks), two different clips, x2_small = 1: seconds equal the oracle's."""
    from lyricalignment_amd import _lib, whisper_compat as wc
    wm = wc.build_model("tiny", seed=4)
    model, dims = _build("tiny", wm)
    audios = [_wave(16000 * 12, 1), _wave(16000 * 12, 2)]
    labels = _labels(2, 11, 9)
    ref_logits, want_ctc, want_plain = _oracle(model, dims, audios, labels)
    with _lib.option("x2_small", 1):
        lg, ctc, plain, two, n = _run(model, audios, labels)
    err = float((lg - ref_logits).abs().max())
    print(f"tiny B=2 x2_small: logits max |err| vs oracle {err:.2e}, {n} small-kernel launches")
    assert n >= 4 * 4 and err < 1e-3
    assert ctc == want_ctc and plain == want_plain and two == want_ctc
