"""Host-side plumbing over the C ABI: torch tensors in, kernels enqueued on the
current HIP stream.  Every wrapper validates shapes / dtypes / contiguity on the
host before a hand-written kernel is launched.  No arithmetic happens here.
"""
from __future__ import annotations

import ctypes
import os
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import (EPI_BIAS, EPI_GELU, EPI_GELU_ERF, EPI_MISH, EPI_OUT_F32, EPI_RESIDUAL, LA_BF16, LA_F32, LA_VARIANT_CTC,
                   LA_VARIANT_PLAIN, check, dtype_code, lib, ptr, stream_ptr)


# The float32 training forward of the attention on the f16 matrix pipe at float32 accuracy (la_attention_lse_f16x2;
# csrc/la_attention_f16x2.hip): sequences of at least 128 queries and keys.  LA_ATTN_F16X2=0 keeps the float32-MFMA kernel (A/B partner).
ATTN_F16X2 = os.environ.get("LA_ATTN_F16X2", "1") != "0"


def _dev(t: torch.Tensor, name: str, dtype=None):
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")


def _capacity(t: torch.Tensor) -> int:
    """Elements addressable from t.data_ptr() to the end of its storage."""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


# --------------------------------------------------------------------------- #
# alignment DP                                                                  #
# --------------------------------------------------------------------------- #
def _lattice_inputs(who: str, em: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, n_frames: torch.Tensor, **more_i32):
    """The checks every lattice entry point makes of em [B,T,E] / labels [B,Lmax] / n_labels [B] / n_frames [B] (and that the
    entry's further int32 device tensors are such) -> B, T, Lmax and the contiguous count tensors."""
    _dev(em, "em", torch.float32); _dev(labels, "labels", torch.int32)
    _dev(n_labels, "n_labels", torch.int32); _dev(n_frames, "n_frames", torch.int32)
    for name, t in more_i32.items():
        _dev(t, name, torch.int32)
    if em.dim() != 3 or labels.dim() != 2 or em.stride(2) != 1 or labels.stride(1) != 1:
        raise ValueError(f"{who}: em [B,T,E] / labels [B,Lmax] with unit inner stride expected")
    B, T, E = em.shape
    Lmax = labels.shape[1]
    if labels.shape[0] != B or n_labels.shape != (B,) or n_frames.shape != (B,) or E < Lmax + 1:
        raise ValueError(f"{who}: inconsistent shapes")
    return B, T, Lmax, n_labels.contiguous(), n_frames.contiguous()


def _lattice_workspace(query: str, B: int, T: int, Lmax: int, device, *more) -> Tuple[torch.Tensor, int]:
    """lib().la_<query>(B, T, Lmax, *more) -> a device byte buffer of max(need, 16) bytes and `need`."""
    need = ctypes.c_size_t(0)
    check(getattr(lib(), "la_" + query)(B, T, Lmax, *more, ctypes.byref(need)), query)
    return torch.empty((max(need.value, 16),), dtype=torch.uint8, device=device), need.value


LINES_MAX_LABELS = 4095
MIN_DURATION_MAX_FRAMES = 8

# One row per C lattice entry (csrc/la_lattice.h Face chooses the kernel; here only what the Python side must know): the stem of its C
# symbols (la_<stem>_batch for a DP, la_<stem> for a sweep, la_<stem>_workspace_bytes), whether it takes the span arguments (skip_from,
# skip_stride, skip_penalty), the window arguments (win_lo, win_hi, win_stride; null = no windows where the public function lets them
# be None) and the repeat / path arguments, whether a sweep writes the span outputs (present_prob, span_skip_prob), and the label limit
# the Python side refuses beyond (NotImplementedError before a launch; None: the C entry's own).  The entries of csrc/la_lattice_tile.h
# take instead one [B, >= Lmax] int32 tensor `row` with its pitch and one `scalar`: a penalty >= 0, or with scalar_max an integer
# 1 .. scalar_max (None: scalar_max) that the workspace query is asked with as well; a DP of theirs writes a path unless told not to, a
# sweep takes a path and writes visits, in_order and path_prob.
class _Entry(NamedTuple):
    stem: str
    spans: bool = False
    windows: bool = False
    repeats: bool = False
    span_out: bool = False
    max_labels: Optional[int] = None
    row: Optional[str] = None
    scalar: Optional[str] = None
    scalar_max: Optional[int] = None


_ENTRIES = {e.stem: e for e in (
    _Entry("viterbi"), _Entry("viterbi_spans", True), _Entry("viterbi_windows", True, True), _Entry("viterbi_lattice", True, True),
    _Entry("viterbi_repeats", True, True, True),
    _Entry("alignment_posteriors"), _Entry("alignment_posteriors_spans", True, span_out=True),
    _Entry("alignment_posteriors_windows", True, True, span_out=True), _Entry("alignment_posteriors_lattice", True, True, span_out=True),
    _Entry("alignment_posteriors_repeats", True, True, True, True, 511), _Entry("alignment_posteriors_song", True, True, True, True, 4095))}
# the entries of csrc/la_lattice_tile.h: the same rows in a table of their own (_ENTRIES stays the eleven faces of la_lattice.h)
_TILE_ENTRIES = {e.stem: e for e in (
    _Entry("viterbi_lines", max_labels=LINES_MAX_LABELS, row="line_start", scalar="line_jump_penalty"),
    _Entry("viterbi_min_duration", max_labels=LINES_MAX_LABELS, row="min_frames", scalar="max_min_frames", scalar_max=MIN_DURATION_MAX_FRAMES),
    _Entry("alignment_posteriors_lines", max_labels=LINES_MAX_LABELS, row="line_start", scalar="line_jump_penalty"))}


def _entry(stem: str) -> _Entry:
    return _ENTRIES.get(stem) or _TILE_ENTRIES[stem]


_LABEL_LIMIT_WHY = {511: "the repeat lattice's posteriors are one lane per state", 4095: "8192 lattice states per workgroup"}


def _wide_enough(who: str, name: str, t, B: int, least: str, n: int):
    """An optional int32 device tensor [B, >= n] with unit inner stride (least: how the message names n)."""
    if t is not None:
        _dev(t, name, torch.int32)
        if t.dim() != 2 or t.shape[0] != B or t.shape[1] < n or t.stride(1) != 1:
            raise ValueError(f"{who}: {name} [B, >= {least}] with unit inner stride expected")


def _lattice_checked(who: str, e: _Entry, em, labels, n_labels, n_frames, skip_from, skip_penalty, win_lo, win_hi, repeat_from, repeat_penalty,
                     frames=None, path=None, boundary_window=None, row=None, scalar=None):
    """_lattice_inputs plus the checks of the entry's own arguments (frames = the (onset, offset) the posteriors are asked about)
    -> B, T, Lmax, the contiguous count tensors, skip_penalty as a float, the windows as a pair or None, repeat_penalty as a float, the
    entry's scalar as the C call takes it."""
    if (win_lo is None) != (win_hi is None):
        raise ValueError(f"{who}: win_lo and win_hi go together")
    windows = None if win_lo is None else (win_lo, win_hi)
    more = {} if frames is None else dict(onset=frames[0], offset=frames[1])
    if windows is not None:
        more.update(win_lo=win_lo, win_hi=win_hi)
    if skip_from is not None:
        more["skip_from"] = skip_from
    if e.row:
        more[e.row] = row
    B, T, Lmax, n_labels, n_frames = _lattice_inputs(who, em, labels, n_labels, n_frames, **more)
    if frames is not None and (frames[0].shape != (B, Lmax) or frames[1].shape != (B, Lmax)):
        raise ValueError(f"{who}: onset / offset must be [B,Lmax]")
    for t in windows or ():
        if t.dim() != 2 or t.shape[0] != B or t.shape[1] < 2 * Lmax + 1 or t.stride(1) != 1 or t.stride(0) != win_lo.stride(0):
            raise ValueError(f"{who}: win_lo / win_hi [B, >= 2*Lmax+1] with unit inner stride and one row pitch expected")
    if skip_from is not None and (skip_from.dim() != 2 or skip_from.shape[0] != B or skip_from.shape[1] < Lmax + 1 or skip_from.stride(1) != 1):
        raise ValueError(f"{who}: skip_from [B, >= Lmax+1] with unit inner stride expected")
    if e.row:                               # (a tile entry answers for its tensors before its numbers, a repeat entry after them)
        _wide_enough(who, e.row, row, B, "Lmax", Lmax)
        _wide_enough(who, "path", path, B, "T", T)
    if boundary_window is not None and int(boundary_window) < 0:
        raise ValueError(f"{who}: boundary_window must be >= 0")
    skip_penalty = float(skip_penalty)
    if e.spans and not skip_penalty >= 0.0:
        raise ValueError(f"{who}: skip_penalty must be >= 0")
    if not e.row:
        _wide_enough(who, "repeat_from", repeat_from, B, "Lmax", Lmax)
        _wide_enough(who, "path", path, B, "T", T)
    repeat_penalty = float(repeat_penalty)
    if e.repeats and not repeat_penalty >= 0.0:
        raise ValueError(f"{who}: repeat_penalty must be >= 0")
    if e.scalar_max is not None:
        scalar = e.scalar_max if scalar is None else int(scalar)
        if not 1 <= scalar <= e.scalar_max:
            raise ValueError(f"{who}: {e.scalar} must be 1 .. {e.scalar_max}")
    elif e.scalar:
        scalar = float(scalar)
        if not scalar >= 0.0:
            raise ValueError(f"{who}: {e.scalar} must be >= 0")
    if e.max_labels is not None and Lmax > e.max_labels:
        raise NotImplementedError(f"{who}: max_labels {Lmax} exceeds {e.max_labels} ({_LABEL_LIMIT_WHY[e.max_labels]})")
    return B, T, Lmax, n_labels, n_frames, skip_penalty, windows, repeat_penalty, scalar


def _face_args(e: _Entry, skip_from, skip_stride: int, skip_penalty: float, windows, repeat_from, repeat_penalty: float, row=None,
               scalar=None) -> tuple:
    """The C arguments an entry adds to the plain one's: (skip_from, skip_stride, skip_penalty), (win_lo, win_hi, win_stride) -- null and 0
    without windows -- and (repeat_from, repeat_stride, repeat_penalty); a tile entry's (row, row_stride, scalar)."""
    lo, hi = windows or (None, None)
    return (((ptr(skip_from), skip_stride, skip_penalty) if e.spans else ())
            + ((ptr(lo), ptr(hi), lo.stride(0) if lo is not None else 0) if e.windows else ())
            + ((ptr(repeat_from), repeat_from.stride(0) if repeat_from is not None else 0, repeat_penalty) if e.repeats else ())
            + ((ptr(row), row.stride(0), scalar) if e.row else ()))


def _viterbi(stem: str, em, labels, n_labels, n_frames, skip_from=None, skip_penalty=0.0, win_lo=None, win_hi=None, repeat_from=None,
             repeat_penalty=0.0, row=None, scalar=None, want_path=True):
    """The alignment DP through one entry: checks, outputs, workspace and the C call -> onset, offset, final_score, status [, path]."""
    e, who = _entry(stem), stem + "_batch"
    B, T, Lmax, n_labels, n_frames, skip_penalty, windows, repeat_penalty, scalar = _lattice_checked(
        who, e, em, labels, n_labels, n_frames, skip_from, skip_penalty, win_lo, win_hi, repeat_from, repeat_penalty, row=row, scalar=scalar)
    dev = em.device
    onset, offset = (torch.empty((B, Lmax), dtype=torch.int32, device=dev) for _ in range(2))
    score = torch.empty((B,), dtype=torch.float64, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    has_path = e.repeats or bool(e.row)
    path = torch.empty((B, T), dtype=torch.int32, device=dev) if has_path and want_path else None
    ws, need = _lattice_workspace(stem + "_workspace_bytes", B, T, Lmax, dev, *((scalar,) if e.scalar_max is not None else ()))
    skip_stride = skip_from.stride(0) if skip_from is not None else 0
    check(getattr(lib(), "la_" + who)(
        ptr(em), em.stride(0), em.stride(1), ptr(labels), labels.stride(0), ptr(n_labels), ptr(n_frames), B, T, Lmax,
        ptr(onset), ptr(offset), Lmax, ptr(score), ptr(status),
        *_face_args(e, skip_from, skip_stride, skip_penalty, windows, repeat_from, repeat_penalty, row, scalar),
        *((ptr(path), T if path is not None else 0) if has_path else ()), ptr(ws), need, stream_ptr()), who)
    return (onset, offset, score, status, path) if has_path else (onset, offset, score, status)


def _posteriors(who: str, em, labels, n_labels, n_frames, onset, offset, boundary_window, want_gamma, skip_from=None, skip_penalty=0.0,
                win_lo=None, win_hi=None, repeat_from=None, repeat_penalty=0.0, path=None, row=None, scalar=None):
    """The forward-backward sweep through one entry (`who`, the stem of its C symbols): checks, outputs, workspace and the C call ->
    occupancy, onset_prob, offset_prob, log_z, status [, present_prob, span_skip_prob [, repeat_count, path_prob]] [, gamma]; a tile
    entry: ..., status, visits, in_order, path_prob [, gamma]."""
    e = _entry(who)
    B, T, Lmax, n_labels, n_frames, skip_penalty, windows, repeat_penalty, scalar = _lattice_checked(
        who, e, em, labels, n_labels, n_frames, skip_from, skip_penalty, win_lo, win_hi, repeat_from, repeat_penalty, (onset, offset), path,
        boundary_window, row, scalar)
    onset = onset.contiguous(); offset = offset.contiguous()
    dev = em.device
    occupancy, onset_prob, offset_prob = (torch.empty((B, Lmax), dtype=torch.float32, device=dev) for _ in range(3))
    log_z = torch.empty((B,), dtype=torch.float64, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    gamma = torch.empty((B, T, 2 * Lmax + 1), dtype=torch.float32, device=dev) if want_gamma else None
    more = ()                               # what the entry writes beside the plain five, in the C call's order and the result's
    skip_stride = skip_from.stride(0) if skip_from is not None else Lmax + 1
    if e.span_out:                          # skip_stride is the row pitch the kernel is told for skip_from AND for span_skip_prob
        present_prob = torch.empty((B, Lmax), dtype=torch.float32, device=dev)          # (`visits` on the repeat lattice)
        more = (present_prob, torch.empty((B, max(skip_stride, Lmax + 1)), dtype=torch.float32, device=dev)[:, :Lmax + 1])
    path_prob = torch.empty((B, path.stride(0)), dtype=torch.float32, device=dev)[:, :T] if path is not None else None   # the row pitch of path
    if e.repeats:
        more += (torch.empty((B, Lmax), dtype=torch.float32, device=dev), path_prob)
    if e.row:                               # visits, in_order
        more += tuple(torch.empty((B, Lmax), dtype=torch.float32, device=dev) for _ in range(2)) + (path_prob,)
    ws, need = _lattice_workspace(who + "_workspace_bytes", B, T, Lmax, dev)
    check(getattr(lib(), "la_" + who)(
        ptr(em), em.stride(0), em.stride(1), ptr(labels), labels.stride(0), ptr(n_labels), ptr(n_frames), B, T, Lmax,
        ptr(onset), ptr(offset), Lmax, int(boundary_window),
        *_face_args(e, skip_from, skip_stride, skip_penalty, windows, repeat_from, repeat_penalty, row, scalar),
        *((ptr(path), path.stride(0) if path is not None else 0) if e.repeats or e.row else ()),
        ptr(occupancy), ptr(onset_prob), ptr(offset_prob), *(ptr(t) for t in more), ptr(log_z), ptr(status), ptr(gamma),
        gamma.stride(0) if want_gamma else 0, gamma.stride(1) if want_gamma else 0, ptr(ws), need, stream_ptr()), who)
    res = (occupancy, onset_prob, offset_prob, log_z, status) + more
    return res + (gamma,) if want_gamma else res


def viterbi_batch(em: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, n_frames: torch.Tensor
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """em [B,T,E] f32 (E >= Lmax+1), labels [B,Lmax] i32, n_labels [B] i32, n_frames [B] i32 (device).
    -> onset [B,Lmax] i32, offset [B,Lmax] i32, final_score [B] f64, status [B] i32 (device)."""
    return _viterbi("viterbi", em, labels, n_labels, n_frames)


def viterbi_spans_batch(em: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, n_frames: torch.Tensor,
                        skip_from: torch.Tensor, skip_penalty: float = 0.0
                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """la_viterbi_spans_batch: viterbi_batch on the lattice with optional label spans.  skip_from [B, >= Lmax+1] i32 (device):
    skip_from[b, n] = a (0 <= a < n) makes labels a..n-1 of clip b optional, anything else = no span ends at n.
    -> the tuple of viterbi_batch; labels inside a taken jump have onset = offset = -1 under status LA_OK."""
    return _viterbi("viterbi_spans", em, labels, n_labels, n_frames, skip_from, skip_penalty)


def viterbi_windows_batch(em: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, n_frames: torch.Tensor,
                          win_lo: torch.Tensor, win_hi: torch.Tensor, skip_from: Optional[torch.Tensor] = None, skip_penalty: float = 0.0
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """la_viterbi_windows_batch: viterbi_spans_batch (skip_from None: viterbi_batch) on the lattice with a frame window per state.
    win_lo / win_hi [B, >= 2*Lmax+1] i32 (device, one row pitch): state s of clip b may hold the path at frame t only if
    win_lo[b, s] <= t < win_hi[b, s].  -> the tuple of viterbi_batch; a clip without a path inside its windows has status
    LA_EINFEASIBLE, score -inf and every onset / offset -1."""
    return _viterbi("viterbi_windows", em, labels, n_labels, n_frames, skip_from, skip_penalty, win_lo, win_hi)


def viterbi_lattice_batch(em: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, n_frames: torch.Tensor,
                          skip_from: Optional[torch.Tensor] = None, skip_penalty: float = 0.0, win_lo: Optional[torch.Tensor] = None,
                          win_hi: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """la_viterbi_lattice_batch: the DP on the lattice that skip_from (None: no span) and win_lo / win_hi (both None: no windows)
    describe, for up to 4095 labels.  Up to 511 labels the outputs are viterbi_windows_batch's, viterbi_spans_batch's or viterbi_batch's
    bit for bit, according to what is given.  -> the tuple of viterbi_batch."""
    return _viterbi("viterbi_lattice", em, labels, n_labels, n_frames, skip_from, skip_penalty, win_lo, win_hi)


def viterbi_repeats_batch(em: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, n_frames: torch.Tensor,
                          skip_from: Optional[torch.Tensor] = None, skip_penalty: float = 0.0, win_lo: Optional[torch.Tensor] = None,
                          win_hi: Optional[torch.Tensor] = None, repeat_from: Optional[torch.Tensor] = None, repeat_penalty: float = 0.0
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """la_viterbi_repeats_batch: viterbi_lattice_batch on the lattice with REPEATABLE label spans, for up to 4095 labels.  repeat_from
    [B, >= Lmax] i32 (device): repeat_from[b, a] = e (a < e <= L_b) lets the path of clip b return to label a after label e-1, any number
    of times, each return charged repeat_penalty; anything else (-1) = no repeat span starts at a.  None or all -1: onset, offset, score
    and status are viterbi_lattice_batch's bit for bit.
    -> onset, offset (a label's FIRST visit in time), final_score, status, path [B,T] i32 (the lattice state at every frame t < T_b;
    -1 for t >= T_b and for a clip whose status is LA_EEMPTY or LA_EINVAL or that has no path inside its windows)."""
    return _viterbi("viterbi_repeats", em, labels, n_labels, n_frames, skip_from, skip_penalty, win_lo, win_hi, repeat_from, repeat_penalty)


def viterbi_lines_batch(em: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, n_frames: torch.Tensor, line_start: torch.Tensor,
                        line_jump_penalty: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """la_viterbi_lines_batch: viterbi_batch on the lattice of an unmarked sheet, whose lines may be sung in any order, any number of
    times or not at all, for up to 4095 labels.  line_start [B, >= Lmax] i32 (device): nonzero = the label begins a line; entry 0 of a
    clip must be nonzero (LA_EINVAL for that clip otherwise).  line_jump_penalty >= 0 (inf allowed) is charged per jump between lines,
    per start at another line than the first and per end at another line than the last; it has not been tuned on real singing.
    -> onset, offset (a label's FIRST visit in time; -1 for a label never visited, under status LA_OK), final_score, status, path [B,T]
    i32 (the lattice state at every frame t < T_b; -1 for t >= T_b and for a clip whose status is LA_EEMPTY or LA_EINVAL)."""
    return _viterbi("viterbi_lines", em, labels, n_labels, n_frames, row=line_start, scalar=line_jump_penalty)


def viterbi_min_duration_batch(em: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, n_frames: torch.Tensor, min_frames: torch.Tensor,
                               max_min_frames: Optional[int] = None, want_path: bool = True):
    """la_viterbi_min_duration_batch: viterbi_batch on the plain lattice with a floor under every character's duration, for up to 4095
    labels.  min_frames [B, >= Lmax] i32 (device): label n of clip b lasts at least min_frames[b, n] frames, 1 .. max_min_frames; a clip
    with an entry outside that range gets LA_EINVAL.  max_min_frames (1 .. 8; None: 8, nothing is read back from the device) is the bound
    on the floors of this call and picks the kernel's chain depth.  With every floor 1 the first four outputs are viterbi_batch's bit for
    bit.  No floor has been tuned on real singing.
    -> onset, offset (offset - onset >= the floor for every reported label), final_score, status, path [B,T] i32 (None without
    want_path; the lattice state at every frame t < T_b, -1 for t >= T_b and for a clip whose status is not LA_OK).  A clip too short for
    its floors has status LA_EINFEASIBLE and every onset / offset -1."""
    return _viterbi("viterbi_min_duration", em, labels, n_labels, n_frames, row=min_frames, scalar=max_min_frames, want_path=want_path)


def alignment_posteriors(em: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, n_frames: torch.Tensor,
                         onset: torch.Tensor, offset: torch.Tensor, boundary_window: int = 2, want_gamma: bool = False):
    """la_alignment_posteriors: forward-backward on the DP's lattice.  em / labels / n_labels / n_frames as viterbi_batch,
    onset / offset [B,Lmax] i32 = viterbi_batch's (or align_head_forward's) outputs for the same emissions.
    -> occupancy, onset_prob, offset_prob [B,Lmax] f32, log_z [B] f64, status [B] i32 [, gamma [B,T,2*Lmax+1] f32] (device)."""
    return _posteriors("alignment_posteriors", em, labels, n_labels, n_frames, onset, offset, boundary_window, want_gamma)


def alignment_posteriors_spans(em: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, n_frames: torch.Tensor,
                               onset: torch.Tensor, offset: torch.Tensor, skip_from: torch.Tensor, skip_penalty: float = 0.0,
                               boundary_window: int = 2, want_gamma: bool = False):
    """la_alignment_posteriors_spans: forward-backward on the lattice with optional label spans.  Inputs as alignment_posteriors, onset /
    offset = viterbi_spans_batch's outputs for the same skip_from [B, >= Lmax+1] i32 and skip_penalty.
    -> occupancy, onset_prob, offset_prob [B,Lmax] f32, log_z [B] f64, status [B] i32, present_prob [B,Lmax] f32 (label n is on the path),
    span_skip_prob [B,Lmax+1] f32 (the span ending at position n is jumped) [, gamma [B,T,2*Lmax+1] f32] (device)."""
    return _posteriors("alignment_posteriors_spans", em, labels, n_labels, n_frames, onset, offset, boundary_window, want_gamma,
                       skip_from, skip_penalty)


def alignment_posteriors_windows(em: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, n_frames: torch.Tensor,
                                 onset: torch.Tensor, offset: torch.Tensor, win_lo: torch.Tensor, win_hi: torch.Tensor,
                                 skip_from: Optional[torch.Tensor] = None, skip_penalty: float = 0.0, boundary_window: int = 2,
                                 want_gamma: bool = False):
    """la_alignment_posteriors_windows: alignment_posteriors_spans (skip_from None: no span anywhere) on the lattice with a frame window
    per state, the lattice of viterbi_windows_batch; onset / offset = its outputs for the same windows, skip_from and skip_penalty.
    win_lo / win_hi as viterbi_windows_batch.  Every output is a posterior GIVEN the windows (normalised by the windowed log_z).
    -> the tuple of alignment_posteriors_spans (skip_from None: present_prob 1 on reported labels, span_skip_prob 0); a clip without a
    path inside its windows has status LA_EINFEASIBLE, log_z -inf and every output 0."""
    return _posteriors("alignment_posteriors_windows", em, labels, n_labels, n_frames, onset, offset, boundary_window, want_gamma,
                       skip_from, skip_penalty, win_lo, win_hi)


def alignment_posteriors_lattice(em: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, n_frames: torch.Tensor,
                                 onset: torch.Tensor, offset: torch.Tensor, skip_from: Optional[torch.Tensor] = None,
                                 skip_penalty: float = 0.0, win_lo: Optional[torch.Tensor] = None, win_hi: Optional[torch.Tensor] = None,
                                 boundary_window: int = 2, want_gamma: bool = False):
    """la_alignment_posteriors_lattice: forward-backward on the lattice that skip_from (None: no span) and win_lo / win_hi (both None: no
    windows) describe, for up to 4095 labels; onset / offset = viterbi_lattice_batch's outputs for the same lattice.  Up to 511 labels the
    outputs are alignment_posteriors_windows', alignment_posteriors_spans' or (the five common ones) alignment_posteriors' bit for bit,
    according to what is given.  The workspace holds every alpha row: B * T * 1024 R * 8 bytes beyond 511 labels (R = 2 / 4 / 8 for up to
    1023 / 2047 / 4095 labels).  -> the tuple of alignment_posteriors_spans (no span: present_prob 1 on the labels of an LA_OK clip,
    span_skip_prob 0)."""
    return _posteriors("alignment_posteriors_lattice", em, labels, n_labels, n_frames, onset, offset, boundary_window, want_gamma,
                       skip_from, skip_penalty, win_lo, win_hi)


def alignment_posteriors_repeats(em: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, n_frames: torch.Tensor,
                                 onset: torch.Tensor, offset: torch.Tensor, skip_from: Optional[torch.Tensor] = None,
                                 skip_penalty: float = 0.0, win_lo: Optional[torch.Tensor] = None, win_hi: Optional[torch.Tensor] = None,
                                 repeat_from: Optional[torch.Tensor] = None, repeat_penalty: float = 0.0,
                                 path: Optional[torch.Tensor] = None, boundary_window: int = 2, want_gamma: bool = False):
    """la_alignment_posteriors_repeats: forward-backward on the lattice of viterbi_repeats_batch, for up to 511 labels
    (NotImplementedError above, before a launch); onset / offset / path = its outputs for the same lattice.  A path may visit a label
    more than once, so visits, onset_prob, offset_prob, repeat_count and (under a repeat span) span_skip_prob are EXPECTED COUNTS that
    can exceed 1; nothing is clamped (include/lyricalign.h).  repeat_from None or all -1: the numbers of alignment_posteriors_lattice
    bit for bit, visits = its present_prob, repeat_count 0.
    -> occupancy, onset_prob, offset_prob [B,Lmax] f32, log_z [B] f64, status [B] i32, visits [B,Lmax] f32, span_skip_prob [B,Lmax+1] f32,
    repeat_count [B,Lmax] f32, path_prob [B,T] f32 (gamma at the given path; None without a path) [, gamma [B,T,2*Lmax+1] f32]."""
    return _posteriors("alignment_posteriors_repeats", em, labels, n_labels, n_frames, onset, offset, boundary_window, want_gamma,
                       skip_from, skip_penalty, win_lo, win_hi, repeat_from, repeat_penalty, path)


def alignment_posteriors_song(em: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, n_frames: torch.Tensor,
                              onset: torch.Tensor, offset: torch.Tensor, skip_from: Optional[torch.Tensor] = None,
                              skip_penalty: float = 0.0, win_lo: Optional[torch.Tensor] = None, win_hi: Optional[torch.Tensor] = None,
                              repeat_from: Optional[torch.Tensor] = None, repeat_penalty: float = 0.0,
                              path: Optional[torch.Tensor] = None, boundary_window: int = 2, want_gamma: bool = False):
    """la_alignment_posteriors_song: alignment_posteriors_repeats for whole songs, up to 4095 labels (NotImplementedError above, before a
    launch); the same arguments and the same tuple.  Up to 511 labels the same kernel and the same bits; beyond, the strip form (R = 2 /
    4 / 8 states per thread for up to 1023 / 2047 / 4095 labels), whose workspace holds every alpha row: B * T * 1024 R * 8 bytes."""
    return _posteriors("alignment_posteriors_song", em, labels, n_labels, n_frames, onset, offset, boundary_window, want_gamma,
                       skip_from, skip_penalty, win_lo, win_hi, repeat_from, repeat_penalty, path)


def alignment_posteriors_lines(em: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, n_frames: torch.Tensor,
                               onset: torch.Tensor, offset: torch.Tensor, line_start: torch.Tensor, line_jump_penalty: float = 0.0,
                               path: Optional[torch.Tensor] = None, boundary_window: int = 2, want_gamma: bool = False):
    """la_alignment_posteriors_lines: forward-backward on the lattice of viterbi_lines_batch, for up to 4095 labels (NotImplementedError
    above, before a launch); onset / offset / path = its outputs for the same line_start [B, >= Lmax] i32 and line_jump_penalty.  A path
    may visit a label any number of times, so visits, in_order, onset_prob and offset_prob are EXPECTED COUNTS that can exceed 1; nothing
    is clamped (include/lyricalign.h).  in_order[a] counts the visits of a line's first label a that begin in print order (0 for every
    other label); visits - in_order there is the expected number of arrivals out of print order.  The workspace holds every alpha row
    and every target's jump term: B * T * 1.5 * (states per workgroup) * 8 bytes.
    -> occupancy, onset_prob, offset_prob [B,Lmax] f32, log_z [B] f64, status [B] i32, visits [B,Lmax] f32, in_order [B,Lmax] f32,
    path_prob [B,T] f32 (gamma at the given path; None without a path) [, gamma [B,T,2*Lmax+1] f32]."""
    return _posteriors("alignment_posteriors_lines", em, labels, n_labels, n_frames, onset, offset, boundary_window, want_gamma, path=path,
                       row=line_start, scalar=line_jump_penalty)


def emissions_from_logits(logits: torch.Tensor, labels: torch.Tensor, n_labels: torch.Tensor, variant: int) -> torch.Tensor:
    """logits [B,T,V] f32 device -> compact emissions [B,T,Lmax+1] f32."""
    _dev(logits, "logits", torch.float32); _dev(labels, "labels", torch.int32); _dev(n_labels, "n_labels", torch.int32)
    if logits.dim() != 3 or logits.stride(2) != 1:
        raise ValueError("emissions_from_logits: logits [B,T,V] with unit inner stride expected")
    B, T, V = logits.shape
    Lmax = labels.shape[1]
    if labels.shape[0] != B or n_labels.shape != (B,) or labels.stride(1) != 1:
        raise ValueError("emissions_from_logits: inconsistent label shapes")
    em = torch.empty((B, T, Lmax + 1), dtype=torch.float32, device=logits.device)
    check(lib().la_emissions_from_logits(ptr(logits), logits.stride(0), logits.stride(1), B, T, V, variant, ptr(labels),
                                         labels.stride(0), ptr(n_labels.contiguous()), Lmax, ptr(em), em.stride(0),
                                         em.stride(1), stream_ptr()), "emissions_from_logits")
    return em


def _readings_inputs(who: str, em_x: torch.Tensor, alt_start: torch.Tensor, n_labels: torch.Tensor):
    """The checks merge_readings and reading_scores share: em_x [B,T,>=1+max_columns] f32, alt_start [B,>=Lmax+1] i32, n_labels [B] i32
    (device, unit inner strides) -> B, T, max_columns (what the expanded rows hold)."""
    _dev(em_x, "em_x", torch.float32); _dev(alt_start, "alt_start", torch.int32); _dev(n_labels, "n_labels", torch.int32)
    if em_x.dim() != 3 or alt_start.dim() != 2 or em_x.stride(2) != 1 or alt_start.stride(1) != 1:
        raise ValueError(f"{who}: em_x [B,T,E] / alt_start [B,Lmax+1] with unit inner stride expected")
    B, T, E = em_x.shape
    if alt_start.shape[0] != B or alt_start.shape[1] < 2 or n_labels.shape != (B,) or E < alt_start.shape[1]:
        raise ValueError(f"{who}: inconsistent shapes")
    return B, T, E - 1


def merge_readings(em_x: torch.Tensor, alt_start: torch.Tensor, n_labels: torch.Tensor, n_frames: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """la_emissions_merge_readings: the expanded compact emissions em_x [B,T,1+columns] f32 (silence, then every position's readings in
    order) folded into the matrix the lattice reads, em [B,T,Lmax+1]: a position's column is log sum exp over its readings (float64,
    rounded once; one reading: copied bit for bit).  alt_start [B,Lmax+1] i32: the CSR rows (columns 1 + alt_start[b,n] ..
    alt_start[b,n+1] are position n's), n_labels / n_frames [B] i32; all on the device.  Rows t >= n_frames[b] and columns beyond
    n_labels[b] are not written (out: a caller's [B,T,>=Lmax+1] tensor, e.g. to keep what it holds there)."""
    who = "merge_readings"
    B, T, max_columns = _readings_inputs(who, em_x, alt_start, n_labels)
    _dev(n_frames, "n_frames", torch.int32)
    Lmax = alt_start.shape[1] - 1
    if n_frames.shape != (B,):
        raise ValueError(f"{who}: inconsistent shapes")
    if out is None:
        out = torch.empty((B, T, Lmax + 1), dtype=torch.float32, device=em_x.device)
    else:
        _dev(out, "out", torch.float32)
        if out.dim() != 3 or out.shape[0] != B or out.shape[1] != T or out.shape[2] < Lmax + 1 or out.stride(2) != 1:
            raise ValueError(f"{who}: out [B,T,>=Lmax+1] with unit inner stride expected")
    check(lib().la_emissions_merge_readings(ptr(em_x), em_x.stride(0), em_x.stride(1), ptr(alt_start), alt_start.stride(0),
                                            ptr(n_labels.contiguous()), ptr(n_frames.contiguous()), B, T, Lmax, max_columns, ptr(out),
                                            out.stride(0), out.stride(1), stream_ptr()), who)
    return out


def reading_scores(em_x: torch.Tensor, alt_start: torch.Tensor, n_labels: torch.Tensor, onset: torch.Tensor, offset: torch.Tensor
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """la_reading_scores: which reading was sung, on the boundaries the DP chose.  em_x / alt_start / n_labels as merge_readings, onset /
    offset [B,Lmax] i32 (a lattice entry's outputs).  -> reading [B,Lmax] i32 (index into the position's readings, 0 = the sheet's own
    class, the smallest index with the largest score; -1 for a skipped position) and col_score [B,columns] f64 (per expanded column the
    sequential float64 sum of its emissions over its position's segment; 0 for a skipped position).  Entries beyond a clip's own labels
    / columns are unspecified."""
    who = "reading_scores"
    B, T, max_columns = _readings_inputs(who, em_x, alt_start, n_labels)
    _dev(onset, "onset", torch.int32); _dev(offset, "offset", torch.int32)
    Lmax = alt_start.shape[1] - 1
    if onset.shape != (B, Lmax) or offset.shape != (B, Lmax):
        raise ValueError(f"{who}: onset / offset must be [B,Lmax]")
    onset = onset.contiguous(); offset = offset.contiguous()
    reading = torch.empty((B, Lmax), dtype=torch.int32, device=em_x.device)
    col_score = torch.empty((B, max_columns), dtype=torch.float64, device=em_x.device)
    check(lib().la_reading_scores(ptr(em_x), em_x.stride(0), em_x.stride(1), ptr(alt_start), alt_start.stride(0),
                                  ptr(n_labels.contiguous()), ptr(onset), ptr(offset), Lmax, B, T, Lmax, max_columns, ptr(col_score),
                                  max_columns, ptr(reading), Lmax, stream_ptr()), who)
    return reading, col_score


MAX_PRONUNCIATION_TOP_K = 16


def segment_class_scores(em_c: torch.Tensor, n_labels: torch.Tensor, onset: torch.Tensor, offset: torch.Tensor, own_col: torch.Tensor,
                         top_k: int = 5, want_scores: bool = False, out=None):
    """la_segment_class_scores: every candidate class summed over the segment the DP gave a position.  em_c [B,T,C] f32 with unit inner
    stride (any row / batch stride: a column window of a wider matrix is taken as it is), n_labels [B] i32, onset / offset [B,Lmax] i32 (a
    lattice entry's outputs), own_col [B,Lmax] i32 (the candidate column of the position's own class, -1 = none); all on the device.
    -> top_col [B,Lmax,top_k] i32, top_score [B,Lmax,top_k] f64 (the largest sequential float64 sums, the largest first, ties to the
    smaller column; -1 / -inf beyond C entries), own_score [B,Lmax] f64, own_rank [B,Lmax] i32 (candidates before the own class; 0 =
    it is the best, -1 = no own class), n_seg_frames [B,Lmax] i32 [, seg_score [B,Lmax,C] f64 with want_scores].  A skipped position
    (onset -1): top_col -1, own_rank -1, zeros elsewhere.  Entries of positions beyond a clip's own labels are not written.
    out: the caller's tensors in that order (seg_score last where want_scores) -- top_col / top_score with one position pitch and
    stride(0) = Lmax * stride(1), the three [B,Lmax] ones with one row pitch -- e.g. to keep what they hold beyond a clip's labels."""
    who = "segment_class_scores"
    for name, t in (("n_labels", n_labels), ("onset", onset), ("offset", offset), ("own_col", own_col)):
        _dev(t, name, torch.int32)
    _dev(em_c, "em_c", torch.float32)
    if em_c.dim() != 3 or em_c.stride(2) != 1 or onset.dim() != 2:
        raise ValueError(f"{who}: em_c [B,T,C] with unit inner stride and onset [B,Lmax] expected")
    B, T, C = em_c.shape
    Lmax = onset.shape[1]
    if onset.shape[0] != B or offset.shape != (B, Lmax) or own_col.shape != (B, Lmax) or n_labels.shape != (B,):
        raise ValueError(f"{who}: inconsistent shapes")
    top_k = int(top_k)
    if top_k < 1:
        raise ValueError(f"{who}: top_k must be >= 1")
    if top_k > MAX_PRONUNCIATION_TOP_K or C > 4095 or Lmax > 4095:
        raise NotImplementedError(f"{who}: top_k {top_k} exceeds {MAX_PRONUNCIATION_TOP_K}, or {C} candidates / {Lmax} labels exceed 4095")
    dev = em_c.device
    if out is None:
        top_col = torch.empty((B, Lmax, top_k), dtype=torch.int32, device=dev)
        top_score = torch.empty((B, Lmax, top_k), dtype=torch.float64, device=dev)
        own_score = torch.empty((B, Lmax), dtype=torch.float64, device=dev)
        own_rank, n_seg = (torch.empty((B, Lmax), dtype=torch.int32, device=dev) for _ in range(2))
        seg = torch.empty((B, Lmax, C), dtype=torch.float64, device=dev) if want_scores else None
    else:
        top_col, top_score, own_score, own_rank, n_seg = out[:5]
        seg = out[5] if want_scores else None
        for name, t, dt, shape in (("top_col", top_col, torch.int32, (B, Lmax, top_k)), ("top_score", top_score, torch.float64, (B, Lmax, top_k)),
                                   ("own_score", own_score, torch.float64, (B, Lmax)), ("own_rank", own_rank, torch.int32, (B, Lmax)),
                                   ("n_seg_frames", n_seg, torch.int32, (B, Lmax))) + ((("seg_score", seg, torch.float64, (B, Lmax, C)),) if want_scores else ()):
            _dev(t, name, dt)
            if tuple(t.shape) != shape or t.stride(-1) != 1:
                raise ValueError(f"{who}: out: {name} {list(shape)} with unit inner stride expected")
        if (top_col.stride() != top_score.stride() or top_col.stride(0) != Lmax * top_col.stride(1)
                or not own_score.stride(0) == own_rank.stride(0) == n_seg.stride(0)):
            raise ValueError(f"{who}: out: top_col / top_score need one position pitch with stride(0) = Lmax * stride(1), own_score / "
                             "own_rank / n_seg_frames one row pitch")
    pitch = own_score.stride(0)                        # the C entry's out_stride: onset / offset share it with the three [B,Lmax] outputs
    if onset.stride() != (pitch, 1) or offset.stride() != (pitch, 1):
        rows = torch.empty((2, B, pitch), dtype=torch.int32, device=dev)
        rows[0, :, :Lmax] = onset
        rows[1, :, :Lmax] = offset
        onset, offset = rows[0, :, :Lmax], rows[1, :, :Lmax]
    if own_col.stride(1) != 1:
        own_col = own_col.contiguous()
    check(lib().la_segment_class_scores(ptr(em_c), em_c.stride(0), em_c.stride(1), ptr(n_labels.contiguous()), ptr(onset), ptr(offset), pitch,
                                        ptr(own_col), own_col.stride(0), B, T, Lmax, C, top_k, ptr(seg),
                                        seg.stride(0) if seg is not None else 0, seg.stride(1) if seg is not None else 0, ptr(top_col),
                                        ptr(top_score), top_col.stride(1), ptr(own_score), ptr(own_rank), ptr(n_seg), stream_ptr()), who)
    res = (top_col, top_score, own_score, own_rank, n_seg)
    return res + (seg,) if want_scores else res


def offsheet_columns(em: torch.Tensor, slot_cols: torch.Tensor, n_slots: torch.Tensor, n_frames: torch.Tensor,
                     penalty: float) -> torch.Tensor:
    """la_emissions_offsheet_columns: the emission of the off-sheet slots, in place.  em [B,T,>=1+Lmax] f32 with unit inner stride (any row /
    batch stride: a column window of a wider matrix is taken as it is) holds log P(silence) in column 0; slot_cols [B,Smax] i32 the
    slots' label positions (0-based, ascending; an entry outside 0 .. Lmax-1 is skipped), n_slots / n_frames [B] i32; all on the device.
    Column 1 + x of every slot x of clip b becomes max(log(-expm1(em[b,t,0])) - penalty, -1000) (float64, rounded once) for t <
    n_frames[b]; nothing else is written.  penalty >= 0 in nats per frame (ValueError otherwise).  -> em."""
    who = "offsheet_columns"
    _dev(em, "em", torch.float32)
    for name, t in (("slot_cols", slot_cols), ("n_slots", n_slots), ("n_frames", n_frames)):
        _dev(t, name, torch.int32)
    if em.dim() != 3 or em.stride(2) != 1 or slot_cols.dim() != 2 or slot_cols.stride(1) != 1:
        raise ValueError(f"{who}: em [B,T,1+Lmax] / slot_cols [B,Smax] with unit inner stride expected")
    B, T, E = em.shape
    if slot_cols.shape[0] != B or n_slots.shape != (B,) or n_frames.shape != (B,) or E < 2 or slot_cols.shape[1] < 1:
        raise ValueError(f"{who}: inconsistent shapes")
    penalty = float(penalty)
    if not penalty >= 0.0:
        raise ValueError(f"{who}: penalty must be >= 0 (nats per frame), not {penalty}")
    if T == 0:
        return em
    check(lib().la_emissions_offsheet_columns(ptr(em), em.stride(0), em.stride(1), ptr(slot_cols), slot_cols.stride(0),
                                              ptr(n_slots.contiguous()), ptr(n_frames.contiguous()), B, T, E - 1, slot_cols.shape[1],
                                              penalty, stream_ptr()), who)
    return em


# --------------------------------------------------------------------------- #
# encoder / head building blocks                                                #
# --------------------------------------------------------------------------- #
def gemm(a: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None, *, bias: Optional[torch.Tensor] = None,
         residual: Optional[torch.Tensor] = None, gelu: bool = False, mish: bool = False, out_f32: bool = False,
         M: Optional[int] = None, lda: Optional[int] = None, batch: int = 1, stride_a: int = 0, stride_c: int = 0,
         stride_r: int = 0, ldc: Optional[int] = None, ldr: Optional[int] = None, out16: Optional[torch.Tensor] = None,
         ln_stats: Optional[torch.Tensor] = None, ln_csum: Optional[torch.Tensor] = None,
         ln_part: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[z][m][n] = epi(sum_k a[z][m][k] w[n][k]).  `a` may be a flat buffer addressed through
    (M, lda, stride_a): that is how the conv-as-GEMM views (overlapping rows) are expressed.
    LayerNorm folded into the neighbouring GEMMs (la_gemm_fused_ln): `out16` = a second, 16-bit copy of the f32 result rows
    (same row pitch / batch stride as out), `ln_part` [N/64, M, 2] = also its per-segment partial row statistics
    (ln_stats_finalize turns them into [M,2]); `ln_stats` [M,2] + `ln_csum` [N] = apply rstd (acc - mean c) before the bias;
    `ln_csum` alone = the same with the row statistics of `a` taken inside the main loop (K % 128 == 0, K >= 256)."""
    _dev(a, "a"); _dev(w, "w")
    dt = dtype_code(w.dtype)
    if a.dtype != w.dtype:
        raise ValueError("gemm: a and w dtypes differ")
    if w.dim() != 2 or not w.is_contiguous():
        raise ValueError("gemm: w must be contiguous [N,K]")
    N, K = w.shape
    if M is None:
        if a.dim() != 2 or a.stride(1) != 1 or a.shape[1] != K:
            raise ValueError("gemm: a must be [M,K] with unit inner stride (or pass M/lda)")
        M, lda = a.shape[0], a.stride(0)
    if _capacity(a) < (batch - 1) * stride_a + (M - 1) * lda + K:
        raise ValueError("gemm: a buffer smaller than the addressed view")
    c_dtype = torch.float32 if (out_f32 or dt == LA_F32) else w.dtype
    if out is None:
        if batch != 1:
            raise ValueError("gemm: batched call needs an explicit out buffer")
        out = torch.empty((M, N), dtype=c_dtype, device=a.device)
    if out.dtype != c_dtype:
        raise ValueError(f"gemm: out must be {c_dtype}")
    ldc = out.stride(-2) if ldc is None else ldc
    if _capacity(out) < (batch - 1) * stride_c + (M - 1) * ldc + N:
        raise ValueError("gemm: out buffer smaller than the addressed view")
    epi = 0
    if bias is not None:
        _dev(bias, "bias", torch.float32)
        if bias.numel() < N:
            raise ValueError("gemm: bias shorter than N")
        epi |= EPI_BIAS
    if residual is not None:
        _dev(residual, "residual", torch.float32)
        ldr = residual.stride(-2) if ldr is None else ldr
        if _capacity(residual) < (batch - 1) * stride_r + (M - 1) * ldr + N:
            raise ValueError("gemm: residual buffer smaller than the addressed view")
        epi |= EPI_RESIDUAL
    if gelu:
        epi |= EPI_GELU
        if gelu == "erf":                # 16-bit results: the erfc-based form instead of the sigmoid fit (LA_EPI_GELU_ERF)
            epi |= EPI_GELU_ERF
    if mish:
        epi |= EPI_MISH
    if c_dtype == torch.float32 and dt != LA_F32:
        epi |= EPI_OUT_F32
    if out16 is not None or ln_stats is not None or ln_csum is not None:
        if out16 is not None:
            _dev(out16, "out16", w.dtype)
            if c_dtype != torch.float32 or _capacity(out16) < (batch - 1) * stride_c + (M - 1) * ldc + N:
                raise ValueError("gemm: out16 accompanies an f32 out of the same layout")
        if ln_part is not None:
            _dev(ln_part, "ln_part", torch.float32)
            if out16 is None or N % 64 or ln_part.numel() < (N // 64) * M * 2 or not ln_part.is_contiguous():
                raise ValueError("gemm: ln_part [N/64, M, 2] goes with out16, N % 64 == 0")
        if ln_stats is not None or ln_csum is not None:      # ln_csum alone: the main loop takes the row statistics itself
            _dev(ln_csum, "ln_csum", torch.float32)
            if ln_csum.numel() < N or batch != 1:
                raise ValueError("gemm: ln_csum [N] expected (batch 1)")
        if ln_stats is not None:
            _dev(ln_stats, "ln_stats", torch.float32)
            if ln_stats.numel() < 2 * M or not ln_stats.is_contiguous():
                raise ValueError("gemm: ln_stats [M,2] expected")
        check(lib().la_gemm_fused_ln(dt, M, N, K, batch, ptr(a), lda, stride_a, ptr(w), ptr(out), ldc, stride_c, ptr(bias),
                                     ptr(residual), ldr or 0, stride_r, epi, ptr(out16), ldc, stride_c, ptr(ln_stats), ptr(ln_csum),
                                     ptr(ln_part), stream_ptr()), "gemm_fused_ln")
        return out
    check(lib().la_gemm(dt, M, N, K, batch, ptr(a), lda, stride_a, ptr(w), ptr(out), ldc, stride_c, ptr(bias),
                        ptr(residual), ldr or 0, stride_r, epi, stream_ptr()), "gemm")
    return out


def ln_stats_finalize(part: torch.Tensor, out: Optional[torch.Tensor] = None, eps: float = 1e-5) -> torch.Tensor:
    """part [slots, M, 2] (mean, sum of squared deviations) of 64-column row segments -> [M,2] (mean, 1/sqrt(var + eps))."""
    _dev(part, "part", torch.float32)
    if part.dim() != 3 or part.shape[2] != 2 or not part.is_contiguous():
        raise ValueError("ln_stats_finalize: [slots, M, 2] expected")
    slots, M, _ = part.shape
    if out is None:
        out = torch.empty((M, 2), dtype=torch.float32, device=part.device)
    if out.shape != (M, 2) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("ln_stats_finalize: bad out buffer")
    check(lib().la_ln_stats_finalize(ptr(part), slots, M, float(eps), ptr(out), stream_ptr()), "ln_stats_finalize")
    return out


def row_stats16(x: torch.Tensor, out: Optional[torch.Tensor] = None, eps: float = 1e-5) -> torch.Tensor:
    """x [M,d] bf16 / f16 rows -> [M,2] f32 (mean, 1/sqrt(var + eps)) per row (two-pass, biased variance like LayerNorm)."""
    _dev(x, "x")
    if x.dim() != 2 or x.stride(1) != 1 or x.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("row_stats16: [M,d] 16-bit rows expected")
    M, d = x.shape
    if out is None:
        out = torch.empty((M, 2), dtype=torch.float32, device=x.device)
    if out.shape != (M, 2) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("row_stats16: bad out buffer")
    check(lib().la_row_stats16(dtype_code(x.dtype), ptr(x), x.stride(0), M, d, float(eps), ptr(out), stream_ptr()), "row_stats16")
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out_dtype: torch.dtype,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _dev(x, "x", torch.float32); _dev(gamma, "gamma", torch.float32); _dev(beta, "beta", torch.float32)
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("layernorm: x must be [M,d] with unit inner stride")
    M, d = x.shape
    if gamma.numel() != d or beta.numel() != d:
        raise ValueError("layernorm: gamma/beta size mismatch")
    if out is None:
        out = torch.empty((M, d), dtype=out_dtype, device=x.device)
    if out.dtype != out_dtype or out.shape != (M, d) or out.stride(1) != 1:
        raise ValueError("layernorm: bad out buffer")
    check(lib().la_layernorm(ptr(x), x.stride(0), M, d, ptr(gamma), ptr(beta), ptr(out), out.stride(0),
                             dtype_code(out_dtype), stream_ptr()), "layernorm")
    return out


def gemm_split(a: torch.Tensor, w: torch.Tensor, hi: torch.Tensor, lo: torch.Tensor, *, bias: Optional[torch.Tensor] = None,
               residual: Optional[torch.Tensor] = None, in_place: bool = False, gelu: bool = False, M: Optional[int] = None,
               lda: Optional[int] = None, batch: int = 1, stride_a: int = 0, stride_c: int = 0, ld: Optional[int] = None,
               ldr: Optional[int] = None, stride_r: int = 0, ln_part: Optional[torch.Tensor] = None) -> None:
    """(hi, lo) <- epi(a w^T) + residual on the SPLIT residual stream of the 16-bit encoder (la_gemm_split): hi = x rounded to the
    operand dtype [M, N] (the next LayerNorm-folded GEMM's raw operand), lo uint8 [M, N] = the remainder in steps of ulp(hi) / 254.
    residual: f32 rows (the stem's positional embedding), or in_place=True: the stream's own rows (x += ...)."""
    _dev(a, "a"); _dev(w, "w"); _dev(hi, "hi", w.dtype); _dev(lo, "lo", torch.uint8)
    if a.dtype != w.dtype or w.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("gemm_split: 16-bit operands of one dtype")
    if w.dim() != 2 or not w.is_contiguous():
        raise ValueError("gemm_split: w must be contiguous [N,K]")
    if residual is not None and in_place:
        raise ValueError("gemm_split: residual is either an f32 array or the stream itself")
    N, K = w.shape
    if M is None:
        if a.dim() != 2 or a.stride(1) != 1 or a.shape[1] != K:
            raise ValueError("gemm_split: a must be [M,K] with unit inner stride (or pass M/lda)")
        M, lda = a.shape[0], a.stride(0)
    if _capacity(a) < (batch - 1) * stride_a + (M - 1) * lda + K:
        raise ValueError("gemm_split: a buffer smaller than the addressed view")
    ld = hi.stride(-2) if ld is None else ld
    need = (batch - 1) * stride_c + (M - 1) * ld + N
    if _capacity(hi) < need or _capacity(lo) < need:
        raise ValueError("gemm_split: hi / lo smaller than the addressed view")
    epi = 0
    if bias is not None:
        _dev(bias, "bias", torch.float32)
        if bias.numel() < N:
            raise ValueError("gemm_split: bias shorter than N")
        epi |= EPI_BIAS
    if residual is not None:
        _dev(residual, "residual", torch.float32)
        ldr = residual.stride(-2) if ldr is None else ldr
        if _capacity(residual) < (batch - 1) * stride_r + (M - 1) * ldr + N:
            raise ValueError("gemm_split: residual buffer smaller than the addressed view")
    if residual is not None or in_place:
        epi |= EPI_RESIDUAL
    if gelu:
        epi |= EPI_GELU
    if ln_part is not None:
        _dev(ln_part, "ln_part", torch.float32)
        if N % 64 or ln_part.numel() < (N // 64) * M * 2 or not ln_part.is_contiguous():
            raise ValueError("gemm_split: ln_part [N/64, M, 2], N % 64 == 0")
    check(lib().la_gemm_split(dtype_code(w.dtype), M, N, K, batch, ptr(a), lda, stride_a, ptr(w), ptr(hi), ptr(lo), ld, stride_c, ptr(bias),
                              ptr(residual), ldr or 0, stride_r, epi, ptr(ln_part), stream_ptr()), "gemm_split")


def split_decode(hi: torch.Tensor, lo: torch.Tensor) -> torch.Tensor:
    """The f32 values a split residual stream (hi 16-bit, lo uint8) stands for -- plain torch, for tests and inspection; the
    kernels decode in registers (la_common.h SplitRes): x = hi + (lo - 128) (128 / 127) 2^(e - SH), e the frexp exponent of hi."""
    hf = hi.float()
    _, e = torch.frexp(hf)
    sh = 16 if hi.dtype == torch.bfloat16 else 19
    if hi.dtype == torch.float16:
        e = e.clamp(min=-13)                       # f16 subnormals share the ulp of the smallest normal binade
    step = torch.tensor(128.0 / 127.0, dtype=torch.float32, device=hi.device)
    return hf + torch.ldexp(torch.addcmul(-128.0 * step, lo.float(), step), e.to(torch.int32) - sh)


def layernorm_split(hi: torch.Tensor, lo: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out_dtype: torch.dtype,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm over rows of a split residual stream (la_layernorm_split)."""
    _dev(hi, "hi"); _dev(lo, "lo", torch.uint8); _dev(gamma, "gamma", torch.float32); _dev(beta, "beta", torch.float32)
    if hi.dtype not in (torch.bfloat16, torch.float16) or hi.dim() != 2 or hi.stride(1) != 1 or lo.shape != hi.shape or lo.stride() != hi.stride():
        raise ValueError("layernorm_split: hi [M,d] 16-bit and lo [M,d] uint8 of one layout expected")
    M, d = hi.shape
    if gamma.numel() != d or beta.numel() != d:
        raise ValueError("layernorm_split: gamma/beta size mismatch")
    if out is None:
        out = torch.empty((M, d), dtype=out_dtype, device=hi.device)
    if out.dtype != out_dtype or out.shape != (M, d) or out.stride(1) != 1:
        raise ValueError("layernorm_split: bad out buffer")
    check(lib().la_layernorm_split(dtype_code(hi.dtype), ptr(hi), ptr(lo), hi.stride(0), M, d, ptr(gamma), ptr(beta), ptr(out), out.stride(0),
                                   dtype_code(out_dtype), stream_ptr()), "layernorm_split")
    return out


def mel_to_rows(mel: torch.Tensor, c_pad: int, dtype: torch.dtype) -> torch.Tensor:
    """mel [B,n_mels,frames] f32 -> [B, frames+2, c_pad] channels-last, zero border rows / pad channels."""
    _dev(mel, "mel", torch.float32)
    if mel.dim() != 3 or mel.stride(2) != 1:
        raise ValueError("mel_to_rows: mel [B,n_mels,frames] with unit inner stride expected")
    B, n_mels, frames = mel.shape
    out = torch.empty((B, frames + 2, c_pad), dtype=dtype, device=mel.device)
    check(lib().la_mel_to_rows(ptr(mel), mel.stride(0), mel.stride(1), B, n_mels, frames, ptr(out), c_pad,
                               dtype_code(dtype), stream_ptr()), "mel_to_rows")
    return out


def cast_bf16(x: torch.Tensor) -> torch.Tensor:
    _dev(x, "x", torch.float32)
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(lib().la_cast_f32_to_bf16(ptr(x), ptr(y), x.numel(), stream_ptr()), "cast_f32_to_bf16")
    return y


def attention(qkv: torch.Tensor, batch: int, frames: int, n_head: int, out: Optional[torch.Tensor] = None, q_log2: bool = False) -> torch.Tensor:
    """qkv [batch*frames, 3*n_head*64] (q pre-scaled by 1/8, or by log2(e)/8 with q_log2 -- 16-bit dtypes, LA_Q_LOG2) ->
    out [batch*frames, n_head*64], same dtype."""
    _dev(qkv, "qkv")
    dt = dtype_code(qkv.dtype)
    d = n_head * 64
    if qkv.dim() != 2 or qkv.stride(1) != 1 or qkv.shape[1] != 3 * d or qkv.shape[0] < batch * frames:
        raise ValueError("attention: qkv must be [>=batch*frames, 3*n_head*64] with unit inner stride")
    if out is None:
        out = torch.empty((qkv.shape[0], d), dtype=qkv.dtype, device=qkv.device)
    if out.dtype != qkv.dtype or out.dim() != 2 or out.shape[1] != d or out.shape[0] < batch * frames or out.stride(1) != 1:
        raise ValueError("attention: bad out buffer")
    check(lib().la_attention(dt | (_lib.LA_Q_LOG2 if q_log2 else 0), ptr(qkv), qkv.stride(0), ptr(out), out.stride(0), batch, frames, n_head,
                             stream_ptr()), "attention")
    return out


def _frame_counts(n_frames: torch.Tensor, batch: int, what: str) -> torch.Tensor:
    """Per-clip frame counts of the ragged entry points: a device int32 [batch] tensor (values are the caller's to keep <= frames: they
    live on the device and are not read back here)."""
    _dev(n_frames, "n_frames", torch.int32)
    if n_frames.shape != (batch,):
        raise ValueError(f"{what}: n_frames must be int32 [{batch}]")
    return n_frames.contiguous()


def logmel_ragged(audio: torch.Tensor, n_samples, consts: torch.Tensor, out_frames: int = 3000, n_mels: int = 80) -> torch.Tensor:
    """la_logmel_ragged_f32_prepared_n: audio [B, Nmax] f32 (device; clip b = the first n_samples[b] samples of row b), n_samples = host
    sequence of ints -> mel [B, n_mels, out_frames] f32 (n_mels = 80 or 128, the count `consts` were built for): each clip's own log-mel (its own reflect padding and -8 floor) in frames
    0 .. n_samples[b] // 160 - 1, zeros after.  Clips of fewer than 201 samples are refused here (the reflect padding needs them)."""
    _dev(audio, "audio", torch.float32); _dev(consts, "consts", torch.uint8)
    if audio.dim() != 2 or not audio.is_contiguous():
        raise ValueError("logmel_ragged: audio must be contiguous [B, Nmax]")
    B, N = audio.shape
    ns = [int(v) for v in n_samples]
    if len(ns) != B:
        raise ValueError("logmel_ragged: one sample count per clip expected")
    if any(v < 201 for v in ns):
        raise ValueError("logmel_ragged: every clip needs more than 200 samples (reflect padding)")
    if any(v > N for v in ns):
        raise ValueError("logmel_ragged: a sample count exceeds the row length")
    if N // 160 > int(out_frames):
        raise ValueError("logmel_ragged: out_frames < Nmax // 160")
    nsd = torch.tensor(ns, dtype=torch.int32).to(audio.device)
    n_mels = int(n_mels)
    if n_mels not in (80, 128):
        raise ValueError(f"logmel_ragged: n_mels = {n_mels}, the kernels are built for 80 or 128")
    mel = torch.empty((B, n_mels, int(out_frames)), dtype=torch.float32, device=audio.device)
    need = ctypes.c_size_t(0)
    check(lib().la_logmel_workspace_bytes_n(n_mels, B, N, ctypes.byref(need)), "logmel_workspace_bytes_n")
    ws = torch.empty((need.value,), dtype=torch.uint8, device=audio.device)
    check(lib().la_logmel_ragged_f32_prepared_n(n_mels, ptr(audio), ptr(nsd), B, N, ptr(consts), ptr(mel), mel.stride(0), mel.stride(1),
                                                int(out_frames), ptr(ws), need.value, stream_ptr()), "logmel_ragged_f32_prepared_n")
    return mel


def gru_layer(gi: torch.Tensor, w_hh: torch.Tensor, b_hh: torch.Tensor, out: Optional[torch.Tensor] = None,
              want_mish: bool = False, out_mish: Optional[torch.Tensor] = None, flag: Optional[torch.Tensor] = None,
              n_frames: Optional[torch.Tensor] = None):
    """gi [B,T,2,3H] f32; w_hh [2,3H,H] (f32 | bf16); b_hh [2,3H] f32 -> out [B,T,2H] (w_hh dtype) [, Mish(out)].
    `out_mish`: caller-owned [B,T,2H] buffer for Mish(out) (implies want_mish); `flag`: caller-owned int32 [1] word the
    kernel sets when one of its bounded waits times out (default: a fresh zeroed one per call).
    `n_frames` (device int32 [B], values <= T): per-clip lengths (la_gru_layer_ragged) -- rows t < n_frames[b] are the clip's own
    recurrence over n_frames[b] frames, rows past them unspecified."""
    _dev(gi, "gi", torch.float32); _dev(w_hh, "w_hh"); _dev(b_hh, "b_hh", torch.float32)
    dt = dtype_code(w_hh.dtype)
    if gi.dim() != 4 or gi.shape[2] != 2 or not gi.is_contiguous() or not w_hh.is_contiguous() or not b_hh.is_contiguous():
        raise ValueError("gru_layer: gi must be contiguous [B,T,2,3H]")
    B, T, _, H3 = gi.shape
    H = H3 // 3
    if w_hh.shape != (2, 3 * H, H) or b_hh.shape != (2, 3 * H):
        raise ValueError("gru_layer: weight shapes do not match gi")
    if out is None:
        out = torch.empty((B, T, 2 * H), dtype=w_hh.dtype, device=gi.device)
    if out.shape != (B, T, 2 * H) or out.dtype != w_hh.dtype or not out.is_contiguous():
        raise ValueError("gru_layer: bad out buffer")
    if out_mish is not None:
        want_mish = True
        if out_mish.shape != out.shape or out_mish.dtype != out.dtype or not out_mish.is_contiguous():
            raise ValueError("gru_layer: bad out_mish buffer")
    elif want_mish:
        out_mish = torch.empty_like(out)
    need = ctypes.c_size_t(0)
    check(lib().la_gru_workspace_bytes(B, T, H, ctypes.byref(need)), "gru_workspace_bytes")
    ws = torch.empty((need.value,), dtype=torch.uint8, device=gi.device)
    if flag is None:
        flag = torch.zeros((1,), dtype=torch.int32, device=gi.device)
    _dev(flag, "flag", torch.int32)
    if n_frames is not None:
        nf = _frame_counts(n_frames, B, "gru_layer")
        check(lib().la_gru_layer_ragged(dt, ptr(gi), ptr(w_hh), ptr(b_hh), ptr(out), ptr(out_mish), B, T, ptr(nf), H, ptr(ws), need.value,
                                        ptr(flag), stream_ptr()), "gru_layer_ragged")
    else:
        check(lib().la_gru_layer(dt, ptr(gi), ptr(w_hh), ptr(b_hh), ptr(out), ptr(out_mish), B, T, H, ptr(ws), need.value,
                                 ptr(flag), stream_ptr()), "gru_layer")
    return (out, out_mish, flag) if want_mish else (out, flag)


def fc_emissions(act: torch.Tensor, w_fc: torch.Tensor, b_fc: torch.Tensor, batch: int, frames: int,
                 labels: torch.Tensor, n_labels: torch.Tensor, variant: int, w_x2=None) -> torch.Tensor:
    """act [batch*frames, 2H] (Mish(GRU out)), w_fc [V,2H], b_fc [V] -> compact emissions [batch, frames, Lmax+1] f32.
    The [batch, frames, V] logits are never materialised.  w_x2 = (planes [V,2,2H] f16, inv_scale [V]) of a float32 w_fc: the normaliser
    product on the f16 matrix pipe at float32 accuracy (la_fc_emissions_x2)."""
    _dev(act, "act"); _dev(w_fc, "w_fc"); _dev(b_fc, "b_fc", torch.float32)
    _dev(labels, "labels", torch.int32); _dev(n_labels, "n_labels", torch.int32)
    dt = dtype_code(w_fc.dtype)
    if act.dtype != w_fc.dtype or act.dim() != 2 or act.stride(1) != 1 or not w_fc.is_contiguous():
        raise ValueError("fc_emissions: act [rows,2H] / w_fc [V,2H] of one dtype expected")
    V, K = w_fc.shape
    if act.shape[1] != K or act.shape[0] < batch * frames or b_fc.numel() != V:
        raise ValueError("fc_emissions: inconsistent shapes")
    Lmax = labels.shape[1]
    if labels.shape[0] != batch or n_labels.shape != (batch,) or labels.stride(1) != 1:
        raise ValueError("fc_emissions: inconsistent label shapes")
    em = torch.empty((batch, frames, Lmax + 1), dtype=torch.float32, device=act.device)
    need = ctypes.c_size_t(0)
    if w_x2 is not None:
        planes, inv = w_x2
        _dev(planes, "w_x2 planes", torch.float16); _dev(inv, "w_x2 scales", torch.float32)
        if dt != LA_F32 or tuple(planes.shape) != (V, 2, K) or not planes.is_contiguous() or inv.numel() != V:
            raise ValueError("fc_emissions: w_x2 goes with float32 operands, planes [V, 2, 2H] contiguous and [V] inverse scales")
        check(lib().la_fc_emissions_x2_workspace_bytes(batch, frames, K, V, Lmax, ctypes.byref(need)), "fc_emissions_x2_workspace_bytes")
        ws = torch.empty((need.value,), dtype=torch.uint8, device=act.device)
        check(lib().la_fc_emissions_x2(ptr(act), act.stride(0), ptr(w_fc), ptr(b_fc), ptr(planes), ptr(inv), batch, frames, K, V, variant, ptr(labels),
                                       labels.stride(0), ptr(n_labels.contiguous()), Lmax, ptr(em), em.stride(0), em.stride(1),
                                       ptr(ws), need.value, stream_ptr()), "fc_emissions_x2")
        return em
    check(lib().la_fc_emissions_workspace_bytes(dt, batch, frames, K, V, Lmax, ctypes.byref(need)), "fc_emissions_workspace_bytes")
    ws = torch.empty((need.value,), dtype=torch.uint8, device=act.device)
    check(lib().la_fc_emissions(dt, ptr(act), act.stride(0), ptr(w_fc), ptr(b_fc), batch, frames, K, V, variant, ptr(labels),
                                labels.stride(0), ptr(n_labels.contiguous()), Lmax, ptr(em), em.stride(0), em.stride(1),
                                ptr(ws), need.value, stream_ptr()), "fc_emissions")
    return em


def attention_ex(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, batch: int, q_len: int, kv_len: int, n_head: int,
                 causal: bool = False, out: Optional[torch.Tensor] = None, lse: Optional[torch.Tensor] = None, x2: bool = False) -> torch.Tensor:
    """General attention for the text decoder: q [batch*q_len, >=d] / k, v [batch*kv_len, >=d] row views (column slices of
    packed projections are fine: only the row pitch and the 16-byte alignment matter), q pre-scaled by 1/8."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        _dev(t, name)
        if t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"attention_ex: {name} must be a 2-D row view with unit inner stride")
    dt = dtype_code(q.dtype)
    d = n_head * 64
    if k.dtype != q.dtype or v.dtype != q.dtype or k.stride(0) != v.stride(0):
        raise ValueError("attention_ex: q/k/v dtypes differ or k and v have different row pitch")
    if q.shape[0] < batch * q_len or k.shape[0] < batch * kv_len or v.shape[0] < batch * kv_len or min(q.shape[1], k.shape[1], v.shape[1]) < d:
        raise ValueError("attention_ex: views smaller than batch*len x n_head*64")
    if out is None:
        out = torch.empty((batch * q_len, d), dtype=q.dtype, device=q.device)
    if lse is None and x2 and q.dtype == torch.float32 and q_len >= 128 and kv_len >= 128:
        # float32 inference on the f16 matrix pipe at float32 accuracy (la_attention_lse_f16x2 without the row statistic)
        need = ctypes.c_size_t(0)
        check(lib().la_attention_f16x2_workspace_bytes(batch, q_len, kv_len, n_head, ctypes.byref(need)), "attention_f16x2_workspace_bytes")
        ws = torch.empty((need.value + 256,), dtype=torch.uint8, device=q.device)
        off = (-ws.data_ptr()) % 256
        check(lib().la_attention_lse_f16x2(ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(0), ptr(out), out.stride(0), batch, q_len, kv_len,
                                           n_head, 1 if causal else 0, None, ws.data_ptr() + off, need.value, stream_ptr()), "attention_lse_f16x2")
        return out
    if lse is not None:                 # float32 training forward: also the row statistic for la_attention_bwd_f32
        _dev(lse, "lse", torch.float32)
        if q.dtype != torch.float32 or lse.numel() < batch * n_head * q_len or not lse.is_contiguous():
            raise ValueError("attention_ex: lse goes with float32 operands, [batch, n_head, q_len] contiguous")
        if ATTN_F16X2 and q_len >= 128 and kv_len >= 128:
            need = ctypes.c_size_t(0)
            check(lib().la_attention_f16x2_workspace_bytes(batch, q_len, kv_len, n_head, ctypes.byref(need)), "attention_f16x2_workspace_bytes")
            ws = torch.empty((need.value + 256,), dtype=torch.uint8, device=q.device)
            off = (-ws.data_ptr()) % 256
            check(lib().la_attention_lse_f16x2(ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(0), ptr(out), out.stride(0), batch, q_len, kv_len,
                                               n_head, 1 if causal else 0, ptr(lse), ws.data_ptr() + off, need.value, stream_ptr()), "attention_lse_f16x2")
            return out
        check(lib().la_attention_lse_f32(ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(0), ptr(out), out.stride(0), batch, q_len, kv_len,
                                         n_head, 1 if causal else 0, ptr(lse), stream_ptr()), "attention_lse")
        return out
    check(lib().la_attention_ex(dt, ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(0), ptr(out), out.stride(0), batch, q_len,
                                kv_len, n_head, 1 if causal else 0, stream_ptr()), "attention_ex")
    return out


def embed_tokens(tokens: torch.Tensor, token_embedding: torch.Tensor, positional_embedding: torch.Tensor) -> torch.Tensor:
    """tokens int64 [B,n] -> f32 [B*n, d] = token_embedding[tokens] + positional_embedding[:n]."""
    _dev(tokens, "tokens", torch.int64); _dev(token_embedding, "token_embedding", torch.float32)
    _dev(positional_embedding, "positional_embedding", torch.float32)
    B, n = tokens.shape
    V, d = token_embedding.shape
    if positional_embedding.shape[0] < n or positional_embedding.shape[1] != d:
        raise ValueError("embed_tokens: positional table too short or width mismatch")
    x = torch.empty((B * n, d), dtype=torch.float32, device=tokens.device)
    check(lib().la_embed_tokens(ptr(tokens.contiguous()), B, n, ptr(token_embedding.contiguous()), V,
                                ptr(positional_embedding.contiguous()), d, ptr(x), stream_ptr()), "embed_tokens")
    return x


def attention_cached(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, batch: int, q_len: int, kv_len: int, n_head: int,
                     q_batch_rows: int, kv_batch_rows: int, causal: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention of the last q_len positions against a key / value cache holding kv_batch_rows (>= kv_len) rows per clip:
    q [batch*q_batch_rows, >= d], k / v [batch*kv_batch_rows, >= d] row views -> out [batch*q_len, d]."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        _dev(t, name)
        if t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"attention_cached: {name} must be a 2-D row view with unit inner stride")
    dt = dtype_code(q.dtype)
    d = n_head * 64
    if k.dtype != q.dtype or v.dtype != q.dtype or k.stride(0) != v.stride(0):
        raise ValueError("attention_cached: q/k/v dtypes differ or k and v have different row pitch")
    if q.shape[0] < (batch - 1) * q_batch_rows + q_len or min(k.shape[0], v.shape[0]) < (batch - 1) * kv_batch_rows + kv_len:
        raise ValueError("attention_cached: views shorter than the addressed rows")
    if out is None:
        out = torch.empty((batch * q_len, d), dtype=q.dtype, device=q.device)
    check(lib().la_attention_cached(dt, ptr(q), q.stride(0), q_batch_rows, ptr(k), ptr(v), k.stride(0), kv_batch_rows, ptr(out),
                                    out.stride(0), batch, q_len, kv_len, n_head, 1 if causal else 0, stream_ptr()), "attention_cached")
    return out


def argmax_rows(x: torch.Tensor) -> torch.Tensor:
    """x [R, C] f32 (row view) -> int64 [R]: index of each row's first maximum."""
    _dev(x, "x", torch.float32)
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("argmax_rows: x must be a 2-D row view with unit inner stride")
    out = torch.empty((x.shape[0],), dtype=torch.int64, device=x.device)
    check(lib().la_argmax_rows_f32(ptr(x), x.stride(0), x.shape[0], x.shape[1], ptr(out), stream_ptr()), "argmax_rows")
    return out


def topk_rows(x: torch.Tensor, k: int):
    """x [R, C] f32 row view -> (values [R,k] f32, indices [R,k] int64, lse [R] f32): the k largest entries of each row in
    descending order and the row's log-sum-exp (log-probability = value - lse)."""
    _dev(x, "x", torch.float32)
    if x.dim() != 2 or x.stride(1) != 1 or not 1 <= k <= min(8, x.shape[1]):
        raise ValueError("topk_rows: x must be a 2-D row view and 1 <= k <= min(8, columns)")
    R = x.shape[0]
    vals = torch.empty((R, k), dtype=torch.float32, device=x.device)
    idx = torch.empty((R, k), dtype=torch.int64, device=x.device)
    lse = torch.empty((R,), dtype=torch.float32, device=x.device)
    check(lib().la_topk_rows_f32(ptr(x), x.stride(0), R, x.shape[1], k, ptr(vals), ptr(idx), ptr(lse), stream_ptr()), "topk_rows")
    return vals, idx, lse


# --------------------------------------------------------------------------- #
# model-level entry points (csrc/la_model.cpp)                                  #
# --------------------------------------------------------------------------- #
def _workspace(nbytes: int, device, cache: Optional[dict], key: str) -> torch.Tensor:
    """A 256-byte aligned device byte buffer of at least `nbytes` (torch's caching allocator aligns to 512 B); kept in `cache`
    (one buffer per stage and engine: uses on one stream are ordered) and regrown when a larger one is asked for."""
    if cache is not None:
        t = cache.get(key)
        if t is not None and t.numel() >= nbytes and t.device == device:
            return t
    t = torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device=device)
    if cache is not None:
        cache[key] = t
    return t


def encoder_forward(weights_c, mel: torch.Tensor, out: torch.Tensor, ws_cache: Optional[dict] = None) -> torch.Tensor:
    """la_encoder_forward: mel [B, n_mels, 3000] f32 -> out [B*1500, d] rows; the whole stem + blocks + ln_post sequence is
    enqueued by ONE C call (whisper_model.embed_audio, module/align_model.py:91)."""
    _dev(mel, "mel", torch.float32); _dev(out, "out")
    if mel.dim() != 3 or mel.shape[2] != 3000 or mel.stride(2) != 1 or mel.shape[1] != weights_c.n_mels:
        raise ValueError("encoder_forward: mel [B, n_mels, 3000] with unit inner stride expected")
    B = mel.shape[0]
    if out.dim() != 2 or out.shape != (B * 1500, weights_c.d) or out.stride(1) != 1:
        raise ValueError("encoder_forward: out must be [B*1500, d] rows")
    need = ctypes.c_size_t(0)
    check(lib().la_encoder_workspace_bytes(ctypes.byref(weights_c), B, ctypes.byref(need)), "encoder_workspace_bytes")
    ws = _workspace(need.value, mel.device, ws_cache, "encoder")
    check(lib().la_encoder_forward(ctypes.byref(weights_c), ptr(mel), mel.stride(0), mel.stride(1), B, ptr(out), out.stride(0),
                                   dtype_code(out.dtype), ptr(ws), ws.numel(), stream_ptr()), "encoder_forward")
    return out


def align_head_forward(weights_c, feats: torch.Tensor, clip_stride_rows: int, batch: int, frames: int, labels: torch.Tensor,
                       n_labels: torch.Tensor, variant: int, flag: torch.Tensor, want_emissions: bool = False,
                       ws_cache: Optional[dict] = None, n_frames: Optional[torch.Tensor] = None):
    """la_align_head_forward: encoder rows -> BiGRU x 2 -> Mish -> fused FC + emission prep -> DP, ONE C call.
    -> (onset, offset, score, status[, emissions]).  n_frames (device int32 [batch], values <= frames): per-clip lengths
    (la_align_head_forward_ragged)."""
    _dev(feats, "feats"); _dev(labels, "labels", torch.int32); _dev(n_labels, "n_labels", torch.int32); _dev(flag, "flag", torch.int32)
    if feats.dim() != 2 or feats.stride(1) != 1 or feats.shape[1] != weights_c.in_dim:
        raise ValueError("align_head_forward: feats must be [rows, in_dim] with unit inner stride")
    if feats.shape[0] < (batch - 1) * clip_stride_rows + frames or labels.shape[0] != batch or n_labels.shape != (batch,) or labels.stride(1) != 1:
        raise ValueError("align_head_forward: inconsistent shapes")
    Lmax = labels.shape[1]
    dev = feats.device
    onset = torch.empty((batch, Lmax), dtype=torch.int32, device=dev)
    offset = torch.empty((batch, Lmax), dtype=torch.int32, device=dev)
    score = torch.empty((batch,), dtype=torch.float64, device=dev)
    status = torch.empty((batch,), dtype=torch.int32, device=dev)
    em = torch.empty((batch, frames, Lmax + 1), dtype=torch.float32, device=dev) if want_emissions else None
    need = ctypes.c_size_t(0)
    check(lib().la_align_head_workspace_bytes(ctypes.byref(weights_c), batch, frames, Lmax, ctypes.byref(need)), "align_head_workspace_bytes")
    ws = _workspace(need.value, dev, ws_cache, "head")
    if n_frames is not None:
        nf = _frame_counts(n_frames, batch, "align_head_forward")
        check(lib().la_align_head_forward_ragged(ctypes.byref(weights_c), ptr(feats), feats.stride(0), clip_stride_rows, batch, frames, ptr(nf), variant,
                                                 ptr(labels), labels.stride(0), ptr(n_labels.contiguous()), Lmax, ptr(onset), ptr(offset), Lmax,
                                                 ptr(score), ptr(status), ptr(em), ptr(ws), ws.numel(), ptr(flag), stream_ptr()),
              "align_head_forward_ragged")
    else:
        check(lib().la_align_head_forward(ctypes.byref(weights_c), ptr(feats), feats.stride(0), clip_stride_rows, batch, frames, variant,
                                          ptr(labels), labels.stride(0), ptr(n_labels.contiguous()), Lmax, ptr(onset), ptr(offset), Lmax,
                                          ptr(score), ptr(status), ptr(em), ptr(ws), ws.numel(), ptr(flag), stream_ptr()), "align_head_forward")
    return (onset, offset, score, status, em) if want_emissions else (onset, offset, score, status)
