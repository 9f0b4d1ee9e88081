"""CPU-only checks of the 128-bin log-mel front end (whisper large-v3 / large-v3-turbo): the host face of the la_logmel_*_n entries
(declared, exported, refusals answered before any device call), the constant tables, the model names, and the pin of the float32
restatement tests/logmel_reference.py that tests/test_gpu_logmel_mels.py holds the device kernel to."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import logmel_reference as lr
from conftest import ROOT

NEW = ("la_logmel_constants_bytes_n", "la_logmel_constants_n", "la_logmel_workspace_bytes_n", "la_logmel_f32_n", "la_logmel_f32_prepared_n",
       "la_logmel_ragged_f32_prepared_n")


def test_logmel_n_entry_points_are_declared_exported_and_check_arguments_on_the_host():
    from lyricalignment_amd import _lib
    text = open(os.path.join(ROOT, "include", "lyricalign.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in lyricalign.h"
        assert name in _lib.SYMBOLS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} not exported"
    L = _lib.lib()
    P = 256                                     # a non-null, 256-byte aligned stand-in pointer: every call below is refused before any device call
    big = 1 << 40
    need, old = ctypes.c_size_t(0), ctypes.c_size_t(0)

    # ---- sizes: 80 is the existing entry's, 128 adds three more 16-row blocks of the padded filter bank [208 bins][16 rows] f32 (the
    # constants carry no tag: which bin count a buffer belongs to is recorded on the host by its address, include/lyricalign.h)
    assert L.la_logmel_constants_bytes(ctypes.byref(old)) == _lib.LA_OK
    assert L.la_logmel_constants_bytes_n(80, ctypes.byref(need)) == _lib.LA_OK and need.value == old.value == (26 * 400 * 16 + 5 * 208 * 16) * 4
    assert L.la_logmel_constants_bytes_n(128, ctypes.byref(need)) == _lib.LA_OK and need.value == old.value + 3 * 208 * 16 * 4
    c128 = need.value
    assert L.la_logmel_constants_bytes_n(128, None) == _lib.LA_EINVAL
    for b, n in ((6, 480000), (3, 201), (1, 160)):
        assert L.la_logmel_workspace_bytes(b, n, ctypes.byref(old)) == _lib.LA_OK
        assert L.la_logmel_workspace_bytes_n(80, b, n, ctypes.byref(need)) == _lib.LA_OK and need.value == old.value
        assert L.la_logmel_workspace_bytes_n(128, b, n, ctypes.byref(need)) == _lib.LA_OK
        assert need.value == old.value + 3 * 208 * 16 * 4                      # (the one-call form keeps its constants there; both are 256-byte multiples)
    assert L.la_logmel_workspace_bytes_n(128, 0, 480000, ctypes.byref(need)) == _lib.LA_EINVAL
    assert L.la_logmel_workspace_bytes_n(128, 6, 159, ctypes.byref(need)) == _lib.LA_EINVAL
    assert L.la_logmel_workspace_bytes_n(128, 6, 480000, None) == _lib.LA_EINVAL
    assert L.la_logmel_workspace_bytes_n(128, 6, 480000, ctypes.byref(need)) == _lib.LA_OK
    ws128 = need.value

    # ---- the five argument lists, all valid but for what a case changes
    calls = {
        "la_logmel_constants_n": (128, P, P, P, c128, 0),
        "la_logmel_f32_n": (128, P, 6, 480000, P, P, P, 128 * 3000, 3000, P, big, 0),
        "la_logmel_f32_prepared_n": (128, P, 6, 480000, P, P, 128 * 3000, 3000, P, big, 0),
        "la_logmel_ragged_f32_prepared_n": (128, P, P, 6, 480000, P, P, 128 * 3000, 3000, 3000, P, big, 0),
    }

    def refused(name, i, v, word=None):
        ok = calls[name]
        rc = getattr(L, name)(*(ok[:i] + (v,) + ok[i + 1:]))
        assert rc == _lib.LA_EINVAL, (name, i, v, rc)
        if word is not None:
            assert word in _lib.last_error(), (name, i, v, _lib.last_error())

    # a bin count the kernels are not built for: the message names the two they are built for
    for bad in (0, 64, 96, 129):
        assert L.la_logmel_constants_bytes_n(bad, ctypes.byref(need)) == _lib.LA_EINVAL and "80 or 128" in _lib.last_error()
        assert L.la_logmel_workspace_bytes_n(bad, 6, 480000, ctypes.byref(need)) == _lib.LA_EINVAL and "80 or 128" in _lib.last_error()
        for name in calls:
            refused(name, 0, bad, "80 or 128")
    # null pointers
    for i in (1, 2, 3):
        refused("la_logmel_constants_n", i, 0, "null")
    refused("la_logmel_constants_n", 4, c128 - 1, "too small")
    refused("la_logmel_constants_n", 4, c128 - 3 * 208 * 16 * 4, "too small")                     # an 80-bin buffer's size
    refused("la_logmel_constants_n", 3, P + 4, "aligned")
    for i in (1, 4, 5, 6, 9):                                                                     # audio, filters, window, mel, workspace
        refused("la_logmel_f32_n", i, 0, "null")
    for i in (1, 5, 8):                                                                           # audio, mel, workspace
        refused("la_logmel_f32_prepared_n", i, 0, "null")
    refused("la_logmel_f32_prepared_n", 4, 0, "constants")
    for i in (1, 6, 10):
        refused("la_logmel_ragged_f32_prepared_n", i, 0, "null")
    refused("la_logmel_ragged_f32_prepared_n", 2, 0, "n_samples")
    refused("la_logmel_ragged_f32_prepared_n", 5, 0, "constants")
    # a workspace that is too small (by one byte; the 80-bin size is too small for 128), a row pitch below the frame count, too few samples
    for name, i in (("la_logmel_f32_n", 10), ("la_logmel_f32_prepared_n", 9), ("la_logmel_ragged_f32_prepared_n", 11)):
        refused(name, i, ws128 - 1, "workspace too small")
        refused(name, i, ws128 - 3 * 208 * 16 * 4, "workspace too small")
    refused("la_logmel_f32_n", 8, 2999, "mel_row_stride")
    refused("la_logmel_f32_prepared_n", 7, 2999, "mel_row_stride")
    refused("la_logmel_ragged_f32_prepared_n", 8, 2999)
    refused("la_logmel_ragged_f32_prepared_n", 9, 2999, "out_frames")
    refused("la_logmel_f32_n", 3, 200, "200 samples")
    refused("la_logmel_f32_prepared_n", 3, 200, "200 samples")
    refused("la_logmel_ragged_f32_prepared_n", 4, 200, "200 samples")
    # constants belong to one bin count: an address la_logmel_constants_n(128, ...) never filled is not taken by a 128-bin call -- the
    # last check, with everything else in order, and still before any launch
    for name in ("la_logmel_f32_prepared_n", "la_logmel_ragged_f32_prepared_n"):
        assert getattr(L, name)(*calls[name]) == _lib.LA_EINVAL and "la_logmel_constants_n(128" in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(L.la_logmel_constants_bytes_n(96, ctypes.byref(need)), "x")


def test_python_surface_refuses_other_bin_counts_before_it_needs_a_device():
    from lyricalignment_amd.audio_frontend import log_mel_spectrogram, log_mel_spectrogram_per_clip
    for bad in (0, 64, 96, 129):
        with pytest.raises(ValueError, match="80 or 128"):
            log_mel_spectrogram(np.zeros(16000, np.float32), n_mels=bad)
        with pytest.raises(ValueError, match="80 or 128"):
            log_mel_spectrogram_per_clip([np.zeros(16000, np.float32)], n_mels=bad)


def test_mel_filter_table_128_matches_transformers():
    """A pin (passes before the 128-bin kernel exists): both host tables are transformers' 128-bin Slaney bank."""
    from transformers.audio_utils import mel_filter_bank
    from lyricalignment_amd.audio_frontend import mel_filter_table
    from oracle import model_oracle as mo
    hf = mel_filter_bank(201, 128, 0.0, 8000.0, 16000, norm="slaney", mel_scale="slaney").T.astype(np.float32)
    assert mel_filter_table(128).shape == (128, 201) and mel_filter_table(128).dtype == np.float32
    np.testing.assert_allclose(mel_filter_table(128), hf, rtol=0, atol=1e-7)
    np.testing.assert_allclose(mo.mel_filters(128), hf, rtol=0, atol=1e-7)
    np.testing.assert_allclose(mel_filter_table(80), mo.mel_filters(80), rtol=0, atol=1e-7)


def test_dims_of_the_large_v3_generation():
    from lyricalignment_amd import whisper_compat as wc
    v3 = wc.dims_for("large-v3")
    assert (v3.n_mels, v3.n_vocab, v3.n_audio_state, v3.n_audio_head, v3.n_audio_layer) == (128, 51866, 1280, 20, 32)
    assert (v3.n_text_state, v3.n_text_head, v3.n_text_layer, v3.n_audio_ctx, v3.n_text_ctx) == (1280, 20, 32, 1500, 448)
    for name in ("turbo", "large-v3-turbo"):
        t = wc.dims_for(name)
        assert (t.n_mels, t.n_vocab, t.n_audio_state, t.n_audio_head, t.n_audio_layer) == (128, 51866, 1280, 20, 32)
        assert (t.n_text_state, t.n_text_head, t.n_text_layer) == (1280, 20, 4)
    for name in ("large", "large-v1", "large-v2"):                             # unchanged: the 80-bin models, "large" among them
        assert wc.dims_for(name) == wc.ModelDimensions(n_mels=80, n_vocab=51865, n_audio_state=1280, n_audio_head=20, n_audio_layer=32,
                                                       n_text_state=1280, n_text_head=20, n_text_layer=32)
    assert wc.dims_for("tiny") == wc.ModelDimensions()
    with pytest.raises(KeyError):
        wc.dims_for("large-v4")


@pytest.mark.parametrize("name", ["large-v3", "turbo"])
def test_key_names_and_shapes_of_the_large_v3_generation_against_transformers(name):
    """tests/test_host_logic.py test_whisper_key_names_and_shapes_against_transformers for the two new sizes, each with its OWN decoder
    depth: a transformers model of these dimensions (meta device), renamed by the Hugging Face <-> upstream table, has exactly the keys
    and shapes of upstream_key_shapes and of this package's container."""
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    from lyricalignment_amd import whisper_compat as wc
    dims = wc.dims_for(name)
    table = wc.upstream_key_shapes(dims)
    assert table["encoder.conv1.weight"] == (1280, 128, 3) and table["decoder.token_embedding.weight"] == (51866, 1280)
    n_dec = 4 if name == "turbo" else 32
    assert len({k.split(".")[2] for k in table if k.startswith("decoder.blocks.")}) == n_dec
    cfg = WhisperConfig(vocab_size=dims.n_vocab, num_mel_bins=dims.n_mels, d_model=dims.n_audio_state, encoder_layers=dims.n_audio_layer,
                        decoder_layers=dims.n_text_layer, encoder_attention_heads=dims.n_audio_head, decoder_attention_heads=dims.n_text_head,
                        encoder_ffn_dim=4 * dims.n_audio_state, decoder_ffn_dim=4 * dims.n_text_state,
                        max_source_positions=dims.n_audio_ctx, max_target_positions=dims.n_text_ctx)
    with torch.device("meta"):
        hf = WhisperForConditionalGeneration(cfg).state_dict()
        ours = wc.Whisper(dims, with_decoder=True)
    up = wc.hf_state_dict_to_upstream(hf)
    assert {k: tuple(v.shape) for k, v in up.items()} == table
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items() if "mask" not in k and "alignment_heads" not in k} == table
    assert {wc.upstream_to_hf_key(k) for k in up} == set(hf) - {"proj_out.weight"}


def test_restatement_is_the_oracle_at_80_and_the_feature_extractor_at_128():
    """tests/logmel_reference.py logmel_ref on tests/test_oracle_model.py's waveform: at 80 bins the oracle's own function bit for bit; at
    128 bins transformers' WhisperFeatureExtractor(feature_size=128) torch path within 2e-5 (test_log_mel_matches_hf_feature_extractor's
    bound for the 80-bin oracle; measured 0.0).  Printed beside it: the float64 form of the same recipe against the float32 one (1.1e-5
    at 128 bins, 6.6e-6 at 80 when this was written), the restatement's own rounding next to the 2e-4 the device kernel is held to."""
    from transformers import WhisperFeatureExtractor
    from oracle import model_oracle as mo
    wav = lr.oracle_test_wave()
    assert torch.equal(lr.logmel_ref(wav, 80), mo.log_mel_spectrogram(wav))
    ours = lr.logmel_ref(wav, 128)
    assert ours.shape == (128, 375) and ours.dtype == torch.float32
    for n in (80, 128):
        gap = float((lr.logmel_ref(wav, n, torch.float64) - lr.logmel_ref(wav, n).double()).abs().max())
        print(f"{n} bins: float32 against float64 restatement {gap:.2e}")      # (a figure for the reader, no bound: -s shows it)
    fe = WhisperFeatureExtractor(feature_size=128)
    hf = fe._torch_extract_fbank_features(wav) if hasattr(fe, "_torch_extract_fbank_features") else None
    if hf is None:
        pytest.skip("HF torch fbank path missing")
    hf = torch.as_tensor(hf)
    hf = hf.reshape(hf.shape[-2], hf.shape[-1])
    err = float((ours - hf[:, : ours.shape[-1]]).abs().max())
    print(f"128 bins: restatement against WhisperFeatureExtractor {err:.2e}")
    np.testing.assert_allclose(ours.numpy(), hf[:, : ours.shape[-1]].numpy(), rtol=0, atol=2e-5)
