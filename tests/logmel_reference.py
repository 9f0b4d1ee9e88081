"""The oracle's log-mel recipe (oracle/model_oracle.py log_mel_spectrogram = whisper.audio.log_mel_spectrogram) restated with the mel bin
count as an argument, and the seeded waveforms the log-mel tests share.  The oracle's own function is the 80-bin form; the large-v3
generation of whisper runs the same recipe over the 128-row filter bank mo.mel_filters(128).

tests/test_host_logmel_mels.py pins logmel_ref(., 128) to transformers' WhisperFeatureExtractor(feature_size=128) and logmel_ref(., 80) to
the oracle's own function; tests/test_gpu_logmel_mels.py holds the device kernel to it."""
import numpy as np
import torch

from oracle import model_oracle as mo

# tests/test_gpu_model.py test_log_mel_ragged_lengths_and_the_one_call_entry_point: both reflect pads inside one 64-frame tile, a partial
# last tile, exactly one tile, one frame past a tile with a remainder of the hop
LENGTHS = (201, 333, 10241, 12345, 64 * 160, 65 * 160 + 159)
# tests/test_gpu_ragged.py: six clips of different lengths and levels (their maxima differ by up to 26 dB)
CLIP_SAMPLES = [60096, 24237, 101760, 48160, 480000, 9000]
CLIP_LEVELS = [1.0, 0.5, 2.0, 0.25, 1.5, 0.1]


def logmel_ref(audio, n_mels: int, dtype=torch.float32) -> torch.Tensor:
    """[.., N] waveform -> [.., n_mels, N // 160]; the -8 floor at the maximum over the WHOLE tensor, as upstream."""
    if not torch.is_tensor(audio):
        audio = torch.from_numpy(np.asarray(audio))
    audio = audio.to(dtype)
    window = torch.hann_window(mo.N_FFT, dtype=dtype)
    stft = torch.stft(audio, mo.N_FFT, mo.HOP_LENGTH, window=window, return_complex=True)
    magnitudes = stft[..., :-1].abs() ** 2
    filters = torch.from_numpy(mo.mel_filters(n_mels)).to(dtype)
    mel_spec = filters @ magnitudes
    log_spec = torch.clamp(mel_spec, min=1e-10).log10()
    log_spec = torch.maximum(log_spec, log_spec.max() - 8.0)
    return (log_spec + 4.0) / 4.0


def wave(n: int, seed: int = 0) -> np.ndarray:
    """tests/test_gpu_model.py's _wave: noise, a 220 Hz tone and a chirp from 3 kHz."""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    return (rs.randn(n) * 0.05 + 0.3 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 3000 * t * (1 + 0.1 * t))).astype(np.float32)


def oracle_test_wave() -> np.ndarray:
    """tests/test_oracle_model.py test_log_mel_matches_hf_feature_extractor's waveform."""
    rs = np.random.RandomState(0)
    t = np.arange(60096) / 16000.0
    return (rs.randn(60096) * 0.05 + 0.3 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 3000 * t)).astype(np.float32)


def clip(i: int) -> np.ndarray:
    """tests/test_gpu_ragged.py's _clip(i, amp) at the levels of its log-mel test."""
    n = CLIP_SAMPLES[i]
    rs = np.random.RandomState(i)
    t = np.arange(n) / 16000.0
    x = rs.randn(n) * 0.05 + 0.3 * np.sin(2 * np.pi * (180 + 40 * i) * t) + 0.2 * np.sin(2 * np.pi * 3000 * t * (1 + 0.1 * t))
    return (CLIP_LEVELS[i] * x).astype(np.float32)
