"""Drop-in for the reference's module/align_model.py (same class names, constructor and method
signatures, attribute names and state_dict key layout), with the inference arithmetic on the
MI355X HIP kernels of liblyricalign_hip.so.

Reference lines mirrored:  RNN  module/align_model.py:11-40;  AlignModel.__init__ :43-70;
frame_manual_forward :72-123;  forward :126-152.

Differences that are deliberate:
  * `audios` may be a list OR a tuple and is never mutated (the reference pads the caller's list
    in place, :78-80, and fails on tuples);
  * the log-mel runs on the device (the reference computes it on the CPU, :84);
  * `compute_dtype` (extra keyword, default float32 = the reference's numerics; torch.bfloat16 / torch.float16 are
    the throughput mode) and `align(...)` (the fused, logits-free fast path) are additions.
There is no PyTorch / CPU fallback: without the HIP library and a gfx950 device these methods raise.
"""
from __future__ import annotations

import math
import os
import weakref
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from .. import _lib, ops
from ..audio_frontend import log_mel_spectrogram, log_mel_spectrogram_per_clip
from ..engine import N_CTX, N_FRAMES, AlignEngine, pack_decoder, pack_encoder, pack_head
from ..whisper_compat import pad_or_trim


def frame_plan(n_mel: int, get_orig_len: bool = True):
    """Host bookkeeping of frame_manual_forward (module/align_model.py:86-115): the 3000-frame mel chunks that go
    through the encoder and how many of each chunk's 1500 output frames are kept.  Python round() = banker's
    rounding, as in the reference (301 -> 150, 303 -> 152).  -> [(start, end, kept_frames)]"""
    if not get_orig_len:
        return [(0, min(n_mel, N_FRAMES), N_CTX)]
    if n_mel <= N_FRAMES:
        return [(0, n_mel, int(round(n_mel / 2.0)))]
    plan = []
    for start in range(0, n_mel, N_FRAMES):
        end = min(start + N_FRAMES, n_mel)
        plan.append((start, end, int(round((end - start) / 2.0))))
    return plan


def song_major_chunks(mel: torch.Tensor, plan) -> torch.Tensor:
    """Long form (:94-105): mel [S,80,n] -> zero-padded 3000-frame chunks ordered song-major, [S*C, 80, 3000].  Every chunk
    but a song's last keeps all of its 1500 output frames, so with this order song s's frames are the contiguous encoder
    output rows s*C*1500 .. +T: the head reads them in place (clip stride C*1500), nothing is concatenated."""
    S, C = mel.shape[0], len(plan)
    assert all(k == N_CTX for _, _, k in plan[:-1])
    out = torch.zeros((S, C, mel.shape[1], N_FRAMES), dtype=mel.dtype, device=mel.device)
    for c, (s0, e0, _) in enumerate(plan):
        out[:, c, :, : e0 - s0] = mel[:, :, s0:e0]
    return out.view(S * C, mel.shape[1], N_FRAMES)


# LA_BRANCH_STREAMS=0: alignment head and text decoder of the training forward / backward on one stream (A/B partner; read at import)
BRANCH_STREAMS = os.environ.get("LA_BRANCH_STREAMS", "1") != "0"

class RNN(nn.Module):
    """GRU(2 layers, bidirectional) -> Mish -> Linear; parameters live in nn.GRU / nn.Linear so the
    state_dict keys are the reference's (align_rnn.rnn.weight_ih_l0 ... align_rnn.fc.bias)."""

    def __init__(self, input_size, hidden_size, output_size, num_layers: int = 2, dropout: float = 0.1,
                 batch_first: bool = True, bidirectional: bool = True) -> None:
        super().__init__()
        self.rnn = nn.GRU(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers, dropout=dropout,
                          batch_first=batch_first, bidirectional=bidirectional)
        self.activate = nn.Mish()
        self.fc = nn.Linear(hidden_size + (bidirectional * hidden_size), output_size)
        self._owner = None

    def forward(self, x):
        if self._owner is None or self._owner() is None:
            raise _lib.LyricAlignHipError("RNN.forward runs through its AlignModel's HIP engine; call it via AlignModel")
        return self._owner()._head_logits(x)


class AlignModel(torch.nn.Module):
    def __init__(self, whisper_model, embed_dim: int = 1280, hidden_dim: int = 384, dropout: float = 0.15,
                 output_dim: int = 10000, bidirectional: bool = True, freeze_encoder: bool = False,
                 train_alignment: bool = True, train_transcript: bool = False, device: str = 'cuda',
                 compute_dtype: torch.dtype = torch.float32) -> None:
        super().__init__()
        self.whisper_model = whisper_model
        self.align_rnn = RNN(input_size=embed_dim, hidden_size=hidden_dim, output_size=output_dim,
                             bidirectional=bidirectional, dropout=dropout)
        self.freeze_encoder = freeze_encoder
        self.train_alignment = train_alignment
        self.train_transcript = train_transcript
        self.device = device
        self.compute_dtype = compute_dtype
        self._engine: Optional[AlignEngine] = None
        self._engine_key = None
        self.align_rnn._owner = weakref.ref(self)
        if hasattr(whisper_model, "_engine_owner"):
            whisper_model._engine_owner = weakref.ref(self)

    # ------------------------------------------------------------------ engine plumbing
    def _n_head(self) -> int:
        dims = getattr(self.whisper_model, "dims", None)
        if dims is not None:
            return int(dims.n_audio_head)
        return int(self.whisper_model.encoder.conv1.weight.shape[0]) // 64

    def _weights_version(self):
        from ..encoder_train import _EPOCH
        return (tuple((p._version, p.data_ptr()) for p in self.parameters())
                + (_EPOCH[0], str(self.compute_dtype), bool(self.train_transcript)))

    def engine(self) -> AlignEngine:
        """Packed device weights; re-packed when parameters were updated (optimizer step, load_state_dict)."""
        key = self._weights_version()
        if self._engine is None or self._engine_key != key:
            dev = self._device()
            enc_sd = {"encoder." + k: v for k, v in self.whisper_model.encoder.state_dict().items()}
            head_sd = {"align_rnn." + k: v for k, v in self.align_rnn.state_dict().items()}
            enc = pack_encoder(enc_sd, self._n_head(), self.compute_dtype, dev)
            head = pack_head(head_sd, self.compute_dtype, dev)
            dec = None
            decoder = getattr(self.whisper_model, "decoder", None)
            if decoder is not None and self.train_transcript:
                dec_sd = {"decoder." + k: v for k, v in decoder.state_dict().items()}
                dec = pack_decoder(dec_sd, int(getattr(self.whisper_model.dims, "n_text_head", self._n_head())), self.compute_dtype, dev)
            self._engine = AlignEngine(enc, head, dev, dec=dec)
            self._engine_key = key
        return self._engine

    def _device(self) -> torch.device:
        _lib.require_gpu()
        dev = torch.device(self.device if self.device != 'cuda' else f'cuda:{torch.cuda.current_device()}')
        if dev.type != "cuda":
            raise _lib.LyricAlignHipError("AlignModel runs on the MI355X only (device must be a cuda/HIP device)")
        return dev

    def _wants_grad(self) -> bool:
        return torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.parameters())

    def _encoder_frozen(self) -> bool:
        """No encoder parameter asks for a gradient.  (The reference's freeze_encoder flag only acts in forward(), :135-139;
        frame_manual_forward back-propagates into whatever still requires grad, and so does this.)"""
        return not any(p.requires_grad for p in self.whisper_model.encoder.parameters())

    def _head_train_logits(self, feats: torch.Tensor, B: int, T: int, stride: int) -> torch.Tensor:
        """Training-mode head (float32, autograd through the HIP forward/backward kernels, inter-layer dropout active)."""
        from ..head_train import HeadFunction, head_params
        d = feats.shape[1]
        x = feats.view(-1, stride, d)[:, :T] if stride != T else feats.view(B, T, d)
        return HeadFunction.apply(x.float(), float(self.align_rnn.rnn.dropout), True, *head_params(self.align_rnn))

    def _encoder_train_features(self, mel: torch.Tensor, get_orig_len: bool) -> torch.Tensor:
        """Trainable-backbone encoder (float32, autograd through the HIP forward/backward kernels): mel -> (embed [B, T, d],
        embed_pad [B, 1500, d]) with the same chunking as the forward-only path (:87-115)."""
        from ..encoder_train import EncoderFunction, encoder_params
        enc = self.whisper_model.encoder
        pos = enc.positional_embedding
        params = encoder_params(enc)
        plan = frame_plan(mel.shape[-1], get_orig_len)
        H = self._n_head()
        if len(plan) == 1:
            embed_pad = EncoderFunction.apply(pad_or_trim(mel, N_FRAMES), pos, H, *params)
            return embed_pad[:, : plan[0][2]], embed_pad
        chunks = [pad_or_trim(mel[:, :, s:e], N_FRAMES) for s, e, _ in plan]
        B = mel.shape[0]
        y = EncoderFunction.apply(torch.cat(chunks, dim=0), pos, H, *params).view(len(chunks), B, N_CTX, -1)
        embed = torch.cat([y[c, :, : plan[c][2]] for c in range(len(chunks))], dim=1)
        return embed, embed[:, :N_CTX]

    def _decoder_train_logits(self, y_in: torch.Tensor, embed_pad: torch.Tensor) -> torch.Tensor:
        """whisper_model.logits(tokens=y_in, audio_features=embed_pad) under autograd (:118-121)."""
        from ..decoder_train import DecoderFunction, decoder_params
        dec = self.whisper_model.decoder
        n_head = int(getattr(self.whisper_model.dims, "n_text_head", self._n_head()))
        return DecoderFunction.apply(y_in.to(embed_pad.device), embed_pad, n_head, *decoder_params(dec))

    def _embed_audio(self, mel: torch.Tensor) -> torch.Tensor:
        """whisper_model.embed_audio: [B,80,3000] -> [B,1500,d] float32."""
        eng = self.engine()
        B = mel.shape[0]
        y = eng.encode(mel, out_dtype=torch.float32)
        return y.view(B, N_CTX, eng.enc.d).clone()

    def _head_logits(self, embed: torch.Tensor) -> torch.Tensor:
        """align_rnn(embed): [B,T,d] -> [B,T,output_dim] float32."""
        eng = self.engine()
        B, T, d = embed.shape
        feats = embed.to(device=eng.device, dtype=self.compute_dtype).contiguous().view(B * T, d)
        out = eng.logits(feats, B, T, T)
        return out

    # ------------------------------------------------------------------ reference API
    def _n_mels(self) -> int:
        """The backbone's mel bin count: 80, or 128 for the large-v3 generation (whisper's ModelDimensions.n_mels)."""
        return int(self.whisper_model.dims.n_mels)

    def _mel_of(self, audios: Sequence[np.ndarray]) -> torch.Tensor:
        max_audio_len = max(map(len, audios))
        batch = np.zeros((len(audios), max_audio_len), dtype=np.float32)   # zero-pad to the batch max (:78-82), no mutation
        for i, a in enumerate(audios):
            batch[i, : len(a)] = np.asarray(a, dtype=np.float32)
        return log_mel_spectrogram(batch, device=self._device(), n_mels=self._n_mels())     # (:84) on the device, with the model's bin count

    def _features(self, mel: torch.Tensor, get_orig_len: bool):
        """-> (feats rows [., d] in compute dtype, B, T, clip stride in rows, embed_pad provider)."""
        eng = self.engine()
        B = mel.shape[0]
        plan = frame_plan(mel.shape[-1], get_orig_len)
        if len(plan) == 1:                                                  # (:87-92) and (:109-115)
            feats = eng.encode(pad_or_trim(mel, N_FRAMES))
            return feats, B, plan[0][2], N_CTX
        # long form (:94-105): non-overlapping 3000-frame chunks, every chunk of every clip in ONE encoder batch
        feats = eng.encode(song_major_chunks(mel, plan))
        return feats, B, sum(k for _, _, k in plan), len(plan) * N_CTX

    def frame_manual_forward(self, audios: List[np.ndarray], y_in=None, get_orig_len: bool = True, mel: Optional[torch.Tensor] = None):
        """(:72-123).  `mel` (addition, training path only): a ready log-mel batch instead of `audios` -- FineTuner.accumulate
        computes it per micro-batch (the reference's log-mel clamps at the BATCH maximum - 8, :84, so a micro-batch's features
        depend on which clips it holds) and runs the micro-batches as one batch from there."""
        train = self._wants_grad()
        if train and not self._encoder_frozen():                            # whole-model fine-tune (train_multitask.py default)
            from ..head_train import HeadFunction, head_params
            if mel is None:
                with torch.no_grad():
                    mel = self._mel_of(audios)
            embed, embed_pad = self._encoder_train_features(mel, get_orig_len)
            align_logit = transcribe_logit = None
            both = self.train_alignment and self.train_transcript and y_in is not None
            # (the GRU time-out flags of this branch are parked and read before its gradients are used: by EncoderFunction.backward in a plain
            # `loss.backward(); optimizer.step()` loop, by FineTuner after its backward -- head_train.CALLER_CHECKS_FLAGS)
            if both and embed.is_cuda and getattr(self, "_branch_streams", True) and BRANCH_STREAMS:
                # The two branches are independent until their losses, and the head's GRU sweeps are 2 x 1500 dependent steps on 12
                # workgroups (13 ms forward, 19 ms backward with the other 244 CUs idle): the head runs on a stream of its own beside
                # the decoder.  autograd runs a node's backward on the stream of its forward and joins the streams where gradients
                # meet (the encoder output), so the backward sweeps overlap the decoder's backward the same way.
                cur = torch.cuda.current_stream(embed.device)
                side = getattr(self, "_head_stream", None)
                if side is None or side.device != embed.device:
                    side = self._head_stream = torch.cuda.Stream(device=embed.device)
                from .. import head_train
                head_train.check_deferred_flags()                           # (of an earlier forward whose backward never ran)
                side.wait_stream(cur)
                head_train.DEFER_FLAG_CHECKS = True                         # the GRU time-out flags are read after the backward: no host
                try:                                                        # synchronisation between the two branches' launches
                    with torch.cuda.stream(side):
                        align_logit = HeadFunction.apply(embed, float(self.align_rnn.rnn.dropout), True, *head_params(self.align_rnn))
                finally:
                    head_train.DEFER_FLAG_CHECKS = False
                embed.record_stream(side)
                transcribe_logit = self._decoder_train_logits(y_in, embed_pad)
                cur.wait_stream(side)
                align_logit.record_stream(cur)
                return align_logit, transcribe_logit
            if self.train_alignment:
                align_logit = HeadFunction.apply(embed, float(self.align_rnn.rnn.dropout), True, *head_params(self.align_rnn))
            if self.train_transcript and y_in is not None:
                transcribe_logit = self._decoder_train_logits(y_in, embed_pad)
            return align_logit, transcribe_logit
        with torch.no_grad():                                               # frozen encoder: forward only
            mel = self._mel_of(audios)
            eng = self.engine()
            feats, B, T, stride = self._features(mel, get_orig_len)
        align_logit = None
        if self.train_alignment:
            if train:
                align_logit = self._head_train_logits(feats, B, T, stride)
            else:
                align_logit = eng.logits(feats, B, T, stride)               # (:106-107, :114-115)
        transcribe_logit = None
        if self.train_transcript and y_in is not None:                      # (:118-121): decoder over embed_pad = first 1500 frames
            embed_pad = feats.view(B, -1, eng.enc.d)[:, :N_CTX].contiguous().view(B * N_CTX, eng.enc.d)
            if train and any(p.requires_grad for p in self.whisper_model.decoder.parameters()):
                transcribe_logit = self._decoder_train_logits(y_in, embed_pad.view(B, N_CTX, -1).float())
            else:
                transcribe_logit = eng.decode(y_in, embed_pad, N_CTX)
        return align_logit, transcribe_logit

    def forward(self, mel, y_in=None):
        if self._wants_grad():                                              # training through forward(): (:135-149)
            from ..encoder_train import EncoderFunction, encoder_params
            from ..head_train import HeadFunction, head_params
            enc = self.whisper_model.encoder
            mel = mel.to(self._device())
            if self.freeze_encoder or self._encoder_frozen():
                with torch.no_grad():
                    embed = self._embed_audio(mel)
            else:
                embed = EncoderFunction.apply(mel, enc.positional_embedding, self._n_head(), *encoder_params(enc))
            align_logit = transcribe_logit = None
            if self.train_alignment:
                align_logit = HeadFunction.apply(embed, float(self.align_rnn.rnn.dropout), True, *head_params(self.align_rnn))
            if self.train_transcript and y_in is not None:
                transcribe_logit = self._decoder_train_logits(y_in, embed)
            return align_logit, transcribe_logit
        eng = self.engine()
        feats = eng.encode(mel)                                             # (:135-139)
        B = mel.shape[0]
        align_logit = eng.logits(feats, B, N_CTX, N_CTX) if self.train_alignment else None
        transcribe_logit = None
        if self.train_transcript and y_in is not None:
            transcribe_logit = eng.decode(y_in, feats, N_CTX)
        return align_logit, transcribe_logit

    # ------------------------------------------------------------------ clips of different lengths, each as if alone (addition)
    def _features_per_clip(self, audios: Sequence[np.ndarray]):
        """-> (feats rows [B*1500, d], B, Tmax, n_frames device int32 [B], T list[int]): ONE log-mel launch set and ONE encoder batch over
        clips of at most 30 s; clip b's log-mel is its own (log_mel_spectrogram_per_clip) and T_b = round(n_mel_b / 2) as frame_plan has it."""
        if audios is None or len(audios) == 0:
            raise ValueError("per_clip: a non-empty sequence of waveforms is expected")
        n_mel = [len(a) // 160 for a in audios]
        if max(n_mel) > N_FRAMES:
            raise ValueError(f"per_clip: clips of more than 30 s ({max(n_mel)} > {N_FRAMES} mel frames) are not batched per clip; "
                             "align them one at a time (the long-form path)")
        eng = self.engine()
        if self._n_mels() != eng.enc.n_mels:                                # (what engine.encode refuses, before the log-mel is launched)
            raise ValueError(f"per_clip: the model's dims.n_mels = {self._n_mels()} but its conv1.weight takes {eng.enc.n_mels} mel bins")
        mel, n_mel = log_mel_spectrogram_per_clip(audios, device=eng.device, out_frames=N_FRAMES, n_mels=self._n_mels())
        T = [frame_plan(n, True)[0][2] for n in n_mel]
        feats = eng.encode(mel)
        return feats, len(T), max(1, max(T)), torch.tensor(T, dtype=torch.int32).to(eng.device), T

    @torch.no_grad()
    def frame_logits_per_clip(self, audios: Sequence[np.ndarray]) -> List[torch.Tensor]:
        """Materialised logits of a ragged batch: list of [T_b, V] float32 device tensors, clip b's being frame_manual_forward([audios[b]])'s
        -- one log-mel launch set, one encoder batch, one head launch set for all clips (the two-step route: perform_viterbi(_ctc) on
        torch.nn.utils.rnn.pad_sequence of them with n_frames=)."""
        feats, B, Tmax, nf, T = self._features_per_clip(audios)
        eng = self.engine()
        out = eng.logits(feats, B, Tmax, N_CTX, n_frames=nf)
        eng.check_gru()
        return [out[b, : T[b]] for b in range(B)]

    # ------------------------------------------------------------------ fused fast path (addition)
    @torch.no_grad()
    def align(self, audios: Optional[Sequence[np.ndarray]] = None, labels=None, *, mel: Optional[torch.Tensor] = None,
              use_ctc: bool = True, hop_size_second: float = 0.02, get_orig_len: bool = True, return_frames: bool = False,
              return_confidence: bool = False, boundary_window: int = 2, per_clip: bool = False, optional_spans=None,
              skip_penalty: float = 0.0, return_span_confidence: bool = False, char_windows=None, onset_anchors=None,
              return_anchored_confidence: bool = False, return_sheet_confidence: bool = False, repeat_spans=None,
              repeat_penalty: float = 0.0, return_segments: bool = False, return_repeat_confidence: bool = False,
              return_song_confidence: bool = False, alternatives=None, return_readings: bool = False,
              min_duration=None, line_starts=None, line_jump_penalty: float = 0.0,
              off_sheet=None, off_sheet_penalty: float = math.log(100), return_off_sheet: bool = False,
              return_line_confidence: bool = False,
              return_pronunciation: bool = False, pronunciation_classes=None, pronunciation_top_k: int = 5):
        """audios (or a ready mel) + class-id labels ([B,Lmax] with -100 padding, or list of lists) ->
        list[B] of list[L] of [onset_s, offset_s], exactly what perform_viterbi(_ctc)(frame_manual_forward(...))
        returns in the reference -- but the [B,T,V] logits are never materialised and nothing leaves the GPU
        except the [L,2] integer frames.
        return_confidence (addition; the reference has no counterpart): -> (seconds, scores), scores[b] = {"occupancy": [L],
        "onset_prob": [L], "offset_prob": [L], "path_log_posterior": float} -- posteriors under the model from the
        forward-backward sweep of the same lattice (ops.alignment_posteriors; boundary_window in frames), not accuracies.
        With return_frames the device tensors: (onset, offset, score, status, occupancy, onset_prob, offset_prob, log_z).
        per_clip (addition; default False = the reference's batch semantics: every waveform zero-padded to the batch maximum before the
        log-mel, one -8 floor and ONE frame count for the whole batch, so a shorter clip's result depends on its batch mates): with True
        clip b's result is what this call returns for [audios[b]] alone -- its own log-mel, T_b = round(n_mel_b / 2) frames, both GRU layers,
        the DP and the posteriors over exactly T_b frames -- while the batch still shares one log-mel launch set, one encoder batch, one
        head launch set and one DP launch.  Needs `audios` (not `mel`), get_orig_len=True and clips of at most 30 s (ValueError).
        optional_spans (addition): optional_spans[b] = list of (a, n) pairs -- labels a .. n-1 of clip b (a lyric line that may not be sung)
        may be left out by the path; the head's emissions go through the DP on the lattice with optional spans (ops.viterbi_spans_batch,
        skip_penalty >= 0 per taken jump) and skipped characters come back as None (onset = offset = -1 with return_frames).  None or
        all-empty: the call as it was.  Not with return_confidence (ValueError; return_span_confidence is the keyword).  Up to 4095 labels
        (beyond 511: ops.viterbi_lattice_batch); the confidence keywords at most 511 (NotImplementedError), return_sheet_confidence excepted.
        return_span_confidence (addition): -> (seconds, scores) on the lattice with optional spans (ops.alignment_posteriors_spans):
        return_confidence's dicts (skipped characters: None in seconds, their three scores 0) plus "sung_prob": [L], the probability that
        the character is on the path at all, and "span_skip_prob": the probability that the span was left out, one value per span of
        optional_spans[b] in the order given.  With return_frames the device tensors (onset, offset, score, status, occupancy, onset_prob,
        offset_prob, log_z, present_prob [B,Lmax], span_skip_prob [B,Lmax+1], indexed by the span's end position).  Without any span:
        return_confidence's numbers, sung_prob 1 and an empty span_skip_prob.
        char_windows / onset_anchors (addition): what is known about time, per clip a list in utils.alignment.windows_from_anchors' form
        -- char_windows[b] = [(n, lo_s, hi_s), ...], onset_anchors[b] = [(n, t_s, tol_s), ...], seconds in the clip's own frames (per_clip and
        the long form included).  The head's emissions go through the DP with a frame window per lattice state (ops.viterbi_windows_batch),
        with or without optional_spans.  None or all-empty: the call as it was.  A clip without a path inside its windows raises like a clip
        too short for its labels (status LA_EINFEASIBLE with return_frames).  Not with return_confidence / return_span_confidence
        (ValueError: return_anchored_confidence is the keyword).  Up to 4095 labels (beyond 511: ops.viterbi_lattice_batch);
        return_anchored_confidence at most 511 (NotImplementedError; return_sheet_confidence takes up to 4095).
        return_anchored_confidence (addition): -> (seconds, scores) on the lattice with the frame windows of char_windows / onset_anchors
        (ops.alignment_posteriors_windows), with or without optional_spans, per_clip and the long form: return_span_confidence's dicts,
        every number a posterior GIVEN the windows, plus "window_log_prob" = log_z(windowed) - log_z(same lattice, no windows) <= 0, the
        log-probability the unanchored model gives to "the path lies inside the windows" (near 0: the anchors agree with the audio;
        strongly negative: one of them fights it; the second log_z is one more launch of the existing sweep).  None or all-empty windows:
        return_span_confidence's dicts and window_log_prob 0.0.  With return_frames the windowed DP's four tensors, then (occupancy,
        onset_prob, offset_prob, log_z, present_prob, span_skip_prob, log_z_free).  A clip without a path inside its windows raises as
        above.  Not together with return_confidence / return_span_confidence (ValueError).
        return_sheet_confidence (addition): whole songs -- return_anchored_confidence's dicts (and, with return_frames, its 11 tensors) for up
        to 4095 labels, with or without optional_spans, onset_anchors / char_windows, per_clip and the long form
        (ops.alignment_posteriors_lattice on the lattice the DP ran on); window_log_prob is 0.0 without windows.  Up to 511 labels the numbers
        are return_anchored_confidence's exactly.  The sweep keeps every alpha row: T * 1024 R * 8 bytes per clip beyond 511 labels (R = 2 /
        4 / 8 for up to 1023 / 2047 / 4095 labels).  Not together with any of the three older confidence keywords (ValueError).
        repeat_spans (addition): repeat_spans[b] = list of (a, e) pairs -- having sung label e-1 of clip b the path may return to label a
        (a chorus printed once and sung twice; ops.viterbi_repeats_batch, repeat_penalty >= 0 per return).  The result keeps its shape: the
        FIRST visit per character, None for a character never visited.  With optional_spans, char_windows / onset_anchors, per_clip and
        the long form, up to 4095 labels; with return_frames the DP's four tensors and path [B, T] (the lattice state per frame).  Not
        with any of the four older confidence keywords (ValueError; return_repeat_confidence is the keyword).  None or all-empty: the call
        as it was.
        return_segments (addition): -> (seconds, segments), segments[b] = the time-ordered list of (char_index, onset_s, offset_s) of EVERY
        visit, with or without repeat_spans.
        return_repeat_confidence (addition): the confidence of the lattice with repeat_spans (ops.alignment_posteriors_repeats on the DP's
        onset / offset / path), with or without optional_spans, onset_anchors / char_windows, per_clip, the long form and return_segments:
        -> (seconds, scores), or (seconds, segments, scores) with return_segments.  A path may visit a character more than once, so some
        numbers are EXPECTED COUNTS that can exceed 1 (nothing is clamped).  scores[b] holds "occupancy", "onset_prob", "offset_prob" [L]
        (about the reported, first visit), "path_log_posterior", "visits" [L] (the expected number of times the character is sung),
        "repeat_count" {(a, e): the expected number of returns} per span of repeat_spans[b], "span_skip_prob" (one value per span of
        optional_spans[b]), "visit_occupancy" (one number per entry of segments[b]: the mean posterior of the reported state over that
        visit's frames) and, where windows are given, "window_log_prob" (from a second sweep without them).  With no repeat span anywhere
        the numbers it shares with return_sheet_confidence are that keyword's exactly.  Up to 511 labels (NotImplementedError before
        anything is launched; return_song_confidence takes whole songs).  With return_frames the DP's four tensors, (occupancy, onset_prob, offset_prob, log_z, visits,
        span_skip_prob [, log_z_free with windows]) and path.  Not together with another confidence keyword (ValueError).
        return_song_confidence (addition): whole songs -- return_repeat_confidence's return, with or without return_segments, for up to 4095
        labels (ops.alignment_posteriors_song), with optional_spans, onset_anchors / char_windows, per_clip and the long form.  Up to 511
        labels its numbers are return_repeat_confidence's exactly.  The sweep keeps every alpha row: T * 1024 R * 8 bytes per clip beyond
        511 labels (R = 2 / 4 / 8 for up to 1023 / 2047 / 4095 labels).  Not together with another confidence keyword (ValueError).
        alternatives (addition): characters with several readings -- alternatives[b] = [(n, [class, ...]), ...]: label n of clip b may also be
        sung as one of these classes (at most 8 readings per position, the sheet's own class included, and at most 4095 expanded columns
        per clip: ValueError / NotImplementedError before anything is launched).  The head runs on the expanded label list, its emissions
        are folded per frame into the merged class, log sum exp over the position's readings (ops.merge_readings), and the lattice runs on
        the folded matrix; two neighbouring positions count as the same label exactly when their reading sets are equal.  With every other
        keyword, per_clip and the long form; occupancy, sung_prob and the other confidences are then posteriors of the merged class.  None
        or all-empty: the call as it was.
        return_readings (addition; with alternatives, ValueError without): the return gains `readings` as its last element (a bare seconds
        becomes (seconds, readings)): readings[b][n] = (class id sung, [score per reading, the sheet's own class first]), None for a skipped
        character; a reading's score is the sum of its emissions over the segment the DP chose (the reported, first visit), the class the
        smallest index with the largest score (ops.reading_scores).  With return_frames two more tensors: reading [B, Lmax] int32 (index
        into the position's readings, -1 = skipped) and col_score [B, columns] float64.
        return_pronunciation / pronunciation_classes / pronunciation_top_k (addition): was the sheet's character the one that was sung?
        The confidences above are posteriors GIVEN the sheet; this is the "goodness of pronunciation" of forced aligners.
        pronunciation_classes (required with return_pronunciation: ValueError without) is an int N -- the classes 1 .. N -- or a sequence of
        class ids; the sheet's own classes (with alternatives every reading's) are unioned in and the list is sorted and unique; label
        columns plus candidates above 4095 raise NotImplementedError before anything is launched.  The head runs ONCE, on the sheet's rows
        (or the expanded ones) followed by the candidate classes; the lattice reads the leading columns of that matrix, and
        ops.segment_class_scores sums every candidate over the segment the DP chose (the reported, first visit), ranks the own class --
        with alternatives the reading ops.reading_scores picked -- and names the pronunciation_top_k (1 .. 16) best.  The return gains
        `pronunciation` as its last element, after `readings`: pronunciation[b][n] = None for a skipped character, else {"class": own class
        id, "frames": n, "log_prob": own_score / n, "rank": candidates that beat the own class (0 = it is the best), "gop": (own_score -
        best score) / n <= 0 (0.0 at rank 0), "top": [(class id, score / n), ...]}.  With every other keyword, per_clip and the long form.
        With return_frames five more tensors, last: top_col [B, Lmax, top_k] int32 (columns of the sorted class list), top_score float64,
        own_score [B, Lmax] float64, own_rank int32, n_seg_frames int32.  Off: the call as it was.  No threshold on gop is calibrated.
        line_starts / line_jump_penalty (addition): an UNMARKED sheet -- the line breaks and nothing else -- whose lines may be sung in any
        order, any number of times or not at all (a sheet prints V1 C V2 B once each; the song sings V1 C V2 C B C).  line_starts[b] =
        [0, 7, 15, ...], the label indices at which a line of clip b begins (ops.viterbi_lines_batch): after the last character of any
        line the path may go on to the first character of any line, it may begin at any line's start and stop at any line's end, each
        such jump charged line_jump_penalty >= 0 (the default 0.0 follows skip_penalty / repeat_penalty and HAS NOT BEEN TUNED on real
        singing).  The result keeps its shape: the FIRST visit per character, None for a character never sung; return_segments gives
        every visit in time order; with return_frames the DP's four tensors and path [B, T].  With per_clip, the long form,
        alternatives / return_readings and return_pronunciation (both read the first visit), up to 4095 labels (NotImplementedError).
        ValueError, before a device is asked for, for a row that does not begin with 0, is not strictly ascending or holds an index >=
        L_b, and together with optional_spans, repeat_spans, onset_anchors, char_windows, off_sheet or any of the six confidence keywords
        above (return_line_confidence is this lattice's).  None: the call as it was.
        return_line_confidence (addition; with line_starts, ValueError without, before a device is asked for): the confidence of the
        lattice with free line order (ops.alignment_posteriors_lines on the DP's onset / offset / path) -> (seconds, scores), or
        (seconds, segments, scores) with return_segments.  A path may sing a line any number of times, so some numbers are EXPECTED
        COUNTS that can exceed 1 (nothing is clamped).  scores[b] holds "occupancy", "onset_prob", "offset_prob" [L] (about the reported,
        first visit; 0 for a character never sung), "path_log_posterior" (of the reported order and timing together), "visits" [L] (the
        expected number of times the character is sung; constant along a line), "visit_occupancy" (one number per entry of segments[b]:
        the mean posterior of the reported state over that visit's frames), "line_visits" [M] (per line the expected number of times it
        is sung: a count, not a probability) and "line_out_of_order" [M] (how many of those are expected to begin out of print order, by
        a jump or a free start).  With per_clip, the long form, alternatives / return_readings and return_pronunciation as far as
        line_starts goes; up to 4095 labels.  With return_frames the DP's four tensors, (occupancy, onset_prob, offset_prob, log_z,
        visits) and path.  The sweep keeps every alpha row and every line start's jump term: T * 1.5 * (states per workgroup) * 8 bytes
        per clip.
        off_sheet / off_sheet_penalty / return_off_sheet (addition): singing that is in the audio but not on the sheet -- ad-libs between
        lines, backing vocals over a break, a spoken intro, an omitted verse, a partial sheet.  off_sheet[b] = [n, ...] puts a SLOT before
        label n of clip b (0 <= n <= L_b; L_b = after the last label): a label position of its own whose emission is log P(frame is not
        silence) - off_sheet_penalty (ops.offsheet_columns on column 0 of the head's matrix), made skippable by a one-label optional span;
        the lattice itself is unchanged.  The slot beats the sheet's character on a frame when that character holds less than
        exp(-off_sheet_penalty) of the voiced probability; the default ln 100 (a 1 % share, in nats per frame) HAS NOT BEEN TUNED on real
        singing.  Every other keyword keeps the caller's numbering (a slot strictly inside an optional or repeat span belongs to it; a
        slot has one reading and no pronunciation entry) and every per-character output keeps its shape; segments name the caller's
        characters.  With per_clip and the long form.  return_off_sheet: the return gains, as its last element, off_sheet[b] = the
        time-ordered list of {"position": n, "onset": s, "offset": s, "frames": k}, one per slot visit -- unused slots are absent, a slot
        under a repeat span may have several; with return_pronunciation each also has "top": [(class id, score per frame), ...]
        (ops.segment_class_scores over the visit: what was heard there).  The confidence keywords that report sung_prob / visits add
        "off_sheet_prob": {n: value} for every slot given, used or not.  Two properties of the lattice: with a slot before the first
        label the first character cannot start at frame 0 (after the last label: the last character cannot end on the last frame); an
        unused slot is charged skip_penalty like every skipped span, so keep off_sheet_penalty above skip_penalty.  ValueError for a
        wrong list count, a bad or repeated n, a slot on a clip without labels, a negative / NaN penalty, and together with
        return_confidence (slots are spans: return_span_confidence is the keyword) or return_frames; NotImplementedError when L_b plus
        its slots exceed 4095 (511 for the confidence keywords that stop there).  None or all-empty: the call as it was.
        min_duration (addition): a floor under every character's duration -- a sung syllable is never one 20 ms frame long, and the plain
        lattice lets it be: a character that is clear at its onset and whose tail sounds like the vowel before it gets a single frame.
        One number of seconds for every character, or per clip a row of per-character seconds (a None row: no floor in that clip); a
        floor is ceil(seconds / hop_size_second - 1e-9) frames, at least 1 and at most 8 (160 ms).  The head's emissions go through the
        DP on the plain lattice with a minimum duration (ops.viterbi_min_duration_batch): every reported character lasts at least its
        floor, the last one included, and a clip too short for its floors raises like one too short for its labels.  With per_clip, the
        long form, alternatives / return_readings (floors belong to positions), return_pronunciation and return_segments, up to 4095
        labels; with return_frames the DP's four tensors and path [B, T].  ValueError, before a device is asked for, for a negative or
        non-finite value, a wrong row count or length or a floor above 8 frames, and together with optional_spans, repeat_spans,
        onset_anchors, char_windows, line_starts, off_sheet or any confidence keyword (this lattice has no posteriors yet).  None, or
        every floor at most one frame: the call as it was, launch for launch.  No floor HAS BEEN TUNED on real singing: no default."""
        from ..utils import alignment as ua
        if return_readings and alternatives is None:
            raise ValueError("align: return_readings goes with alternatives (without them every character has the one reading of its label)")
        if return_anchored_confidence and (return_confidence or return_span_confidence):
            raise ValueError("align: return_anchored_confidence does not go with return_confidence / return_span_confidence (it returns "
                             "their numbers on the windowed lattice)")
        if return_sheet_confidence and (return_confidence or return_span_confidence or return_anchored_confidence):
            raise ValueError("align: return_sheet_confidence does not go with return_confidence / return_span_confidence / "
                             "return_anchored_confidence (it returns their numbers at any size up to 4095 labels)")
        if return_song_confidence and (return_confidence or return_span_confidence or return_anchored_confidence or return_sheet_confidence
                                       or return_repeat_confidence):
            raise ValueError("align: return_song_confidence does not go with another confidence keyword")
        if return_repeat_confidence:
            if return_confidence or return_span_confidence or return_anchored_confidence or return_sheet_confidence:
                raise ValueError("align: return_repeat_confidence does not go with another confidence keyword")
            widest = max((len(l) for l in ua._label_lists(labels, len(labels))), default=0)
            if widest > ua.POSTERIOR_MAX_LABELS:
                raise NotImplementedError(f"align: {widest} labels exceed the {ua.POSTERIOR_MAX_LABELS}-label limit of return_repeat_confidence")
        # minimum duration: every refusal and the rows, before the engine exists
        ua._min_duration_alone("align", min_duration, optional_spans=optional_spans, repeat_spans=repeat_spans, onset_anchors=onset_anchors,
                               char_windows=char_windows, line_starts=line_starts, off_sheet=off_sheet, return_confidence=return_confidence,
                               return_span_confidence=return_span_confidence, return_anchored_confidence=return_anchored_confidence,
                               return_sheet_confidence=return_sheet_confidence, return_repeat_confidence=return_repeat_confidence,
                               return_song_confidence=return_song_confidence, return_line_confidence=return_line_confidence)
        min_frames = ua._min_frames_of("align", min_duration, ua._label_lists(labels, len(labels)), hop_size_second)
        # free line order: the rows and every refusal, before the engine exists
        ua._line_starts_alone("align", line_starts, optional_spans=optional_spans, repeat_spans=repeat_spans, onset_anchors=onset_anchors,
                              char_windows=char_windows, off_sheet=off_sheet, return_confidence=return_confidence,
                              return_span_confidence=return_span_confidence, return_anchored_confidence=return_anchored_confidence,
                              return_sheet_confidence=return_sheet_confidence, return_repeat_confidence=return_repeat_confidence,
                              return_song_confidence=return_song_confidence)
        if return_line_confidence and line_starts is None:
            raise ValueError("align: return_line_confidence is the confidence of the lattice with free line order: it needs line_starts")
        line_start = ua._line_start_of("align", line_starts, ua._label_lists(labels, len(labels)))
        if line_start is not None and not float(line_jump_penalty) >= 0.0:
            raise ValueError("align: line_jump_penalty must be >= 0")
        off = None
        if off_sheet is not None:            # off-sheet slots: from here on the sheet is the expanded one, the keywords are remapped
            off = ua._off_sheet_of("align", off_sheet, off_sheet_penalty, ua._label_lists(labels, len(labels)), optional_spans, repeat_spans,
                                   char_windows, onset_anchors, alternatives,
                                   narrow=return_confidence or return_span_confidence or return_anchored_confidence or return_repeat_confidence)
        if off is not None:
            if return_confidence:
                raise ValueError("align: return_confidence is not defined with off_sheet (a slot is an optional span, and there are no "
                                 "posteriors over the span lattice by that keyword: return_span_confidence=True gives them)")
            if return_frames:
                raise ValueError("align: off_sheet does not go with return_frames (the device tensors are those of the expanded sheet)")
            labels, optional_spans, repeat_spans = off.label_lists, off.optional_spans, off.repeat_spans
            char_windows, onset_anchors, alternatives = off.char_windows, off.onset_anchors, off.alternatives
        rd = None if alternatives is None else ua._readings_of(alternatives, ua._label_lists(labels, len(labels)), keep_empty=return_readings)
        pron = ua._pronunciation_of("align", return_pronunciation, pronunciation_classes, pronunciation_top_k,
                                    ua._label_lists(labels, len(labels)) if return_pronunciation else None, rd,
                                    None if off is None else off.slot_sets())
        eng = self.engine()
        kw = {}
        if per_clip:
            if mel is not None or not get_orig_len:
                raise ValueError("align(per_clip=True) takes waveforms (audios=) and get_orig_len=True")
            feats, B, T, kw["n_frames"], frame_counts = self._features_per_clip(audios)
            stride = N_CTX
        else:
            if mel is None:
                mel = self._mel_of(audios)
            feats, B, T, stride = self._features(mel.to(eng.device), get_orig_len)
            frame_counts = [T] * B
        lab_dev, n_lab, lab_lists = ua._labels_to_device(labels, B, eng.device)
        skip_from = ua._skip_from_of_spans(optional_spans, lab_lists)
        windows = ua._windows_of(char_windows, onset_anchors, lab_lists, frame_counts, hop_size_second)
        if windows is not None and (return_confidence or return_span_confidence):
            raise ValueError("align: char_windows / onset_anchors do not go with return_confidence / return_span_confidence "
                             "(return_anchored_confidence=True gives the posteriors on the windowed lattice)")
        if skip_from is not None and return_confidence:
            raise ValueError("align: return_confidence is not defined with optional_spans (no posteriors over the span lattice by that "
                             "keyword: return_span_confidence=True gives them)")
        confidence = (ua.LINES_CONFIDENCE if return_line_confidence else "song" if return_song_confidence else "repeat" if return_repeat_confidence else "sheet" if return_sheet_confidence
                      else "anchored" if return_anchored_confidence else "span" if return_span_confidence else "plain" if return_confidence
                      else None)
        variant = _lib.LA_VARIANT_CTC if use_ctc else _lib.LA_VARIANT_PLAIN

        def head(lab, n, needed=True):
            # the head is fused with the plain lattice's DP; its emissions leave it only where another lattice or a sweep needs them.  With
            # pronunciation alternatives it runs on the EXPANDED labels for their emissions (with its time-out recovery); its own DP result on
            # that list is meaningless and is dropped without looking at its status.
            # (the anchored confidence runs the plain lattice's DP on the emissions, as perform_viterbi_anchored_scored does: the same
            # bits; the sheet confidence keeps the fused head's, which run_lattice uses only where there is neither a span nor a window)
            out = eng.align_feats_checked(feats, B, T, stride, lab, n, variant, want_emissions=needed, **kw)
            return None if return_anchored_confidence else out[:4], out[4] if needed else None

        out = ua.align_labels("align", head, lab_dev, n_lab, lab_lists, frame_counts, T, kw.get("n_frames"), hop_size_second, confidence,
                              boundary_window, skip_from, windows, skip_penalty, optional_spans, repeat_spans, repeat_penalty, return_segments,
                              alternatives, return_readings, rd, raw=return_frames, pron=pron, off=off, return_off_sheet=return_off_sheet,
                              line_start=line_start, line_jump_penalty=float(line_jump_penalty), min_frames=min_frames)
        if return_frames:                    # 4, 8 (return_confidence), 10 (return_span_confidence) or 11 tensors; 5 with repeat_spans (path);
            r, picked = out
            # reading, col_score behind them, the five tensors of the pronunciation scores last
            return tuple(t for t in r if t is not None) + (() if r.path is None else (r.path,)) + picked
        return out


def encoder_only_engine(whisper_model, mel: torch.Tensor) -> torch.Tensor:
    """embed_audio for a bare whisper_compat.Whisper that is not wrapped in an AlignModel (float32 compute)."""
    _lib.require_gpu()
    cache = getattr(whisper_model, "_la_engine", None)
    from ..encoder_train import _EPOCH
    key = (_EPOCH[0],) + tuple((p._version, p.data_ptr()) for p in whisper_model.encoder.parameters())
    if cache is None or cache[0] != key:
        dev = torch.device(f"cuda:{torch.cuda.current_device()}")
        sd = {"encoder." + k: v for k, v in whisper_model.encoder.state_dict().items()}
        n_head = int(whisper_model.dims.n_audio_head)
        cache = (key, AlignEngine(pack_encoder(sd, n_head, torch.float32, dev), None, dev))
        whisper_model._la_engine = cache
    eng = cache[1]
    return eng.encode(mel, out_dtype=torch.float32).view(mel.shape[0], N_CTX, eng.enc.d).clone()


def decoder_engine_of(whisper_model) -> AlignEngine:
    """The float32 encoder + decoder engine of a bare whisper_compat.Whisper (packed once, re-packed when parameters change)."""
    _lib.require_gpu()
    if whisper_model.decoder is None:
        raise RuntimeError("this Whisper object was built without a decoder")
    cache = getattr(whisper_model, "_la_dec_engine", None)
    from ..encoder_train import _EPOCH
    key = (_EPOCH[0],) + tuple((p._version, p.data_ptr()) for p in whisper_model.parameters())
    if cache is None or cache[0] != key:
        dev = torch.device(f"cuda:{torch.cuda.current_device()}")
        enc_sd = {"encoder." + k: v for k, v in whisper_model.encoder.state_dict().items()}
        dec_sd = {"decoder." + k: v for k, v in whisper_model.decoder.state_dict().items()}
        eng = AlignEngine(pack_encoder(enc_sd, int(whisper_model.dims.n_audio_head), torch.float32, dev), None, dev,
                          dec=pack_decoder(dec_sd, int(whisper_model.dims.n_text_head), torch.float32, dev))
        cache = (key, eng)
        whisper_model._la_dec_engine = cache
    return cache[1]


def decoder_engine(whisper_model, tokens: torch.Tensor, audio_features: torch.Tensor, greedy=None) -> torch.Tensor:
    """Whisper.logits for a bare whisper_compat.Whisper (float32 compute): packs encoder + decoder weights once.
    greedy = (max_new_tokens, eot): run the greedy token loop from the prompt `tokens` instead and return the tokens."""
    eng = decoder_engine_of(whisper_model)
    B, n_audio, d = audio_features.shape
    xa = audio_features.to(device=eng.device, dtype=torch.float32).contiguous().view(B * n_audio, d)
    if greedy is not None and len(greedy) == 3:
        return eng.decode_beam(tokens, xa, greedy[2], greedy[0], greedy[1], n_audio=n_audio)
    if greedy is not None:
        return eng.decode_greedy(tokens, xa, greedy[0], greedy[1], n_audio)
    return eng.decode(tokens, xa, n_audio)
