"""Drop-in for the reference's utils/alignment.py: same function names, arguments, return values and
exception types, with emission prep + the alignment DP + backtrace on the MI355X (la_emissions_from_logits,
la_viterbi_batch, la_viterbi_core).

Reference lines mirrored: perform_viterbi :13-71; run_viterbi_core :73-119; perform_viterbi_ctc :121-188;
get_mae :190-199.  `prediction` may live on the host (the reference hands over `.cpu()` logits) or on the
device (no copy).  Errors: ValueError("<k> is not in list") when a label state is never visited (:183),
IndexError when an utterance has no labels (:152) -- raised for the first offending utterance, like the
reference's per-utterance loop.  No CPU fallback: the HIP library is required.
"""
from __future__ import annotations

import ctypes
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib, ops
from .._lib import LA_EEMPTY, LA_EINFEASIBLE, LA_OK, LA_VARIANT_CTC, LA_VARIANT_PLAIN, check, lib, ptr, stream_ptr


def _label_lists(labels, batch: int) -> List[List[int]]:
    """labels: LongTensor [B,Lmax] with -100 padding, ndarray, or list of lists -> per-utterance class ids (:141)."""
    out = []
    for i in range(batch):
        row = labels[i]
        out.append([int(row[j]) for j in range(len(row)) if int(row[j]) != -100])
    return out


def _labels_to_device(labels, batch: int, device) -> Tuple[torch.Tensor, torch.Tensor, List[List[int]]]:
    lists = _label_lists(labels, batch)
    Lmax = max(1, max((len(l) for l in lists), default=1))
    lab = torch.zeros((batch, Lmax), dtype=torch.int32)
    for b, l in enumerate(lists):
        if l:
            lab[b, : len(l)] = torch.tensor(l, dtype=torch.int32)
    n = torch.tensor([len(l) for l in lists], dtype=torch.int32)
    return lab.to(device), n.to(device), lists


def spans_from_lines(line_lengths: Sequence[int], optional: Sequence[bool]) -> List[int]:
    """One clip's skip_from array (include/lyricalign.h la_viterbi_spans_batch) for lyrics given as consecutive lines of
    line_lengths[i] characters: L + 1 entries, skip_from[end of line i] = start of line i for every line with optional[i], -1 elsewhere."""
    lengths = [int(v) for v in line_lengths]
    if len(lengths) != len(optional):
        raise ValueError("spans_from_lines: one optional flag per line expected")
    if any(v <= 0 for v in lengths):
        raise ValueError("spans_from_lines: every line must hold at least one character")
    skip_from = [-1] * (sum(lengths) + 1)
    a = 0
    for n_chars, opt in zip(lengths, optional):
        if opt:
            skip_from[a + n_chars] = a
        a += n_chars
    return skip_from


def _skip_from_of_spans(optional_spans, label_lists: List[List[int]]):
    """optional_spans[b] = list of (a, n) pairs: labels a .. n-1 of utterance b may be skipped -> host int32 tensor [B, Lmax + 1] of
    skip_from rows (-1 = none), or None when no utterance has a span.  ValueError for a < 0, a >= n, n > L_b or two spans with one end."""
    if optional_spans is None:
        return None
    if len(optional_spans) != len(label_lists):
        raise ValueError(f"optional_spans: {len(label_lists)} span lists expected, one per utterance")
    Lmax = max(1, max((len(l) for l in label_lists), default=1))
    rows = torch.full((len(label_lists), Lmax + 1), -1, dtype=torch.int32)
    any_span = False
    for b, spans in enumerate(optional_spans):
        L = len(label_lists[b])
        for a, n in (spans or ()):
            a, n = int(a), int(n)
            if a < 0 or a >= n or n > L:
                raise ValueError(f"optional_spans[{b}]: span ({a}, {n}) needs 0 <= a < n <= {L}")
            if int(rows[b, n]) >= 0:
                raise ValueError(f"optional_spans[{b}]: two spans end at {n} (one span per end position)")
            rows[b, n] = a
            any_span = True
    return rows if any_span else None


def repeats_from_lines(line_lengths: Sequence[int], repeatable: Sequence[bool]) -> List[int]:
    """One clip's repeat_from array (include/lyricalign.h la_viterbi_repeats_batch) for lyrics given as consecutive lines of
    line_lengths[i] characters: L entries, repeat_from[start of line i] = end of line i for every line with repeatable[i] (the line may
    be sung again right after it was sung), -1 elsewhere."""
    lengths = [int(v) for v in line_lengths]
    if len(lengths) != len(repeatable):
        raise ValueError("repeats_from_lines: one repeatable flag per line expected")
    if any(v <= 0 for v in lengths):
        raise ValueError("repeats_from_lines: every line must hold at least one character")
    repeat_from = [-1] * sum(lengths)
    a = 0
    for n_chars, rpt in zip(lengths, repeatable):
        if rpt:
            repeat_from[a] = a + n_chars
        a += n_chars
    return repeat_from


def _repeat_from_of_spans(repeat_spans, label_lists: List[List[int]]):
    """repeat_spans[b] = list of (a, e) pairs: having sung label e-1 of utterance b the path may return to label a -> host int32 tensor
    [B, Lmax] of repeat_from rows (-1 = none), or None when no utterance has a span.  ValueError for a < 0, a >= e, e > L_b or two spans
    with one start."""
    if repeat_spans is None:
        return None
    if len(repeat_spans) != len(label_lists):
        raise ValueError(f"repeat_spans: {len(label_lists)} span lists expected, one per utterance")
    Lmax = max(1, max((len(l) for l in label_lists), default=1))
    rows = torch.full((len(label_lists), Lmax), -1, dtype=torch.int32)
    any_span = False
    for b, spans in enumerate(repeat_spans):
        L = len(label_lists[b])
        for a, e in (spans or ()):
            a, e = int(a), int(e)
            if a < 0 or a >= e or e > L:
                raise ValueError(f"repeat_spans[{b}]: span ({a}, {e}) needs 0 <= a < e <= {L}")
            if int(rows[b, a]) >= 0:
                raise ValueError(f"repeat_spans[{b}]: two spans start at {a} (one span per start position)")
            rows[b, a] = e
            any_span = True
    return rows if any_span else None


LINES_MAX_LABELS = ops.LINES_MAX_LABELS     # 4095: what the lattice with free line order takes (ops.viterbi_lines_batch)


def lines_from_lengths(line_lengths: Sequence[int]) -> List[int]:
    """One clip's line_start flag row (include/lyricalign.h la_viterbi_lines_batch) for lyrics given as consecutive lines of
    line_lengths[i] characters: L entries, 1 at every line's first character, 0 elsewhere."""
    lengths = [int(v) for v in line_lengths]
    if not lengths or any(v <= 0 for v in lengths):
        raise ValueError("lines_from_lengths: at least one line, and every line must hold at least one character")
    return [flag for n_chars in lengths for flag in [1] + [0] * (n_chars - 1)]


def _line_start_of(who: str, line_starts, label_lists: List[List[int]]):
    """line_starts[b] = the label indices at which a line of utterance b begins, [0, 7, 15, ...] -> host int32 tensor [B, Lmax] of
    line_start flag rows, or None for line_starts None.  ValueError for a wrong row count or a row that does not begin with 0, is not
    strictly ascending or holds an index >= L_b (an utterance without labels takes an empty row); NotImplementedError beyond 4095
    labels.  Nothing here asks for a device."""
    if line_starts is None:
        return None
    if len(line_starts) != len(label_lists):
        raise ValueError(f"{who}: line_starts: {len(label_lists)} rows expected, one per utterance")
    widest = max((len(l) for l in label_lists), default=0)
    if widest > LINES_MAX_LABELS:
        raise NotImplementedError(f"{who}: line_starts: {widest} labels exceed the {LINES_MAX_LABELS}-label limit of the lattice with free line order")
    rows = torch.zeros((len(label_lists), max(1, widest)), dtype=torch.int32)
    for b, row in enumerate(line_starts):
        L = len(label_lists[b])
        row = [] if row is None else list(row)
        if L == 0 and not row:
            continue
        if any(isinstance(v, bool) or int(v) != v for v in row):
            raise ValueError(f"{who}: line_starts[{b}]: label indices expected")
        row = [int(v) for v in row]
        if not row or row[0] != 0 or any(x >= y for x, y in zip(row, row[1:])) or row[-1] >= L:
            raise ValueError(f"{who}: line_starts[{b}] must begin with 0, ascend strictly and stay below the utterance's {L} labels")
        rows[b, row] = 1
    return rows


def _line_starts_alone(who: str, line_starts, **others) -> None:
    """The keywords that do not go with line_starts (others: name -> value as the caller got it; None, False and all-empty lists count as
    not given): ValueError naming both."""
    if line_starts is None:
        return
    for name, value in others.items():
        given = value is not None and value is not False
        if given and isinstance(value, (list, tuple)):
            given = any(bool(row) for row in value)
        if given:
            raise ValueError(f"{who}: line_starts does not go with {name} (the lattice with free line order has the line breaks and nothing "
                             "else: no marked spans, no anchors, no off-sheet slots, no posteriors)")


MIN_DURATION_MAX_FRAMES = ops.MIN_DURATION_MAX_FRAMES     # 8: the deepest floor of the lattice with a minimum duration (ops.viterbi_min_duration_batch): 160 ms


def _min_frames_of(who: str, min_duration, label_lists: List[List[int]], hop_size_second: float):
    """min_duration = one number of seconds for every character, or per utterance a row of per-character seconds (a None row: no floor
    in that utterance) -> host int32 tensor [B, Lmax] of floors in frames, ceil(seconds / hop - 1e-9) and at least 1 (past L_b: 1), or
    None for min_duration None and where every floor is at most one frame: the call as it was.  ValueError for a negative or non-finite
    value, a wrong row count or length, or a floor above MIN_DURATION_MAX_FRAMES frames.  Nothing here asks for a device."""
    if min_duration is None:
        return None
    hop = float(hop_size_second)

    def frames(b, v):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)) or float(v) < 0.0:
            raise ValueError(f"{who}: min_duration{b}: a finite number of seconds >= 0 expected, not {v!r}")
        k = max(1, int(math.ceil(float(v) / hop - 1e-9)))
        if k > MIN_DURATION_MAX_FRAMES:
            raise ValueError(f"{who}: min_duration{b}: {float(v)} s are {k} frames of {hop} s; the floor is at most {MIN_DURATION_MAX_FRAMES} "
                             "frames")
        return k

    rows = torch.ones((len(label_lists), max(1, max((len(l) for l in label_lists), default=1))), dtype=torch.int32)
    if isinstance(min_duration, (list, tuple)) or (isinstance(min_duration, np.ndarray) and min_duration.ndim > 0) or torch.is_tensor(min_duration):
        if len(min_duration) != len(label_lists):
            raise ValueError(f"{who}: min_duration: {len(label_lists)} rows expected, one per utterance (or one number of seconds)")
        for b, row in enumerate(min_duration):
            if row is None:
                continue
            row = row.tolist() if hasattr(row, "tolist") else row
            if not isinstance(row, (list, tuple)) or len(row) != len(label_lists[b]):
                raise ValueError(f"{who}: min_duration[{b}]: {len(label_lists[b])} values expected, one per character")
            if row:
                rows[b, : len(row)] = torch.tensor([frames(f"[{b}]", v) for v in row], dtype=torch.int32)
    else:
        k = frames("", min_duration.item() if hasattr(min_duration, "item") else min_duration)
        for b, l in enumerate(label_lists):
            rows[b, : len(l)] = k
    return rows if int(rows.max()) > 1 else None


def _min_duration_alone(who: str, min_duration, **others) -> None:
    """The keywords that do not go with min_duration (others: name -> value as the caller got it; None, False and all-empty lists count as
    not given): ValueError naming both."""
    if min_duration is None:
        return
    for name, value in others.items():
        given = value is not None and value is not False
        if given and isinstance(value, (list, tuple)):
            given = any(bool(row) for row in value)
        if given:
            raise ValueError(f"{who}: min_duration does not go with {name} (the floor exists on the plain lattice alone: no spans, no "
                             "anchors, no line order, no off-sheet slots, no posteriors)")


MAX_READINGS = 8                # readings per label position, the sheet's own class included
MAX_READING_COLUMNS = 4095      # expanded columns per clip: what the head, the prep and the fold take
READING_SET_ID = 1 << 24        # lattice id of a clip's k-th distinct multi-reading set: READING_SET_ID + k (class ids lie far below)


class Readings(NamedTuple):
    """_readings_of's result (host): what the route with pronunciation alternatives needs beside the labels."""
    labels_x: torch.Tensor          # [B, Xmax] int32: the expanded label rows -- every position's readings in order, the sheet's class first
    alt_start: torch.Tensor         # [B, Lmax + 1] int32: CSR rows into them (alt_start[b, n] .. alt_start[b, n+1]); past L_b the last value
    lattice_ids: torch.Tensor       # [B, Lmax] int32: what the lattice compares -- equal exactly where the reading SETS are equal
    n_columns: List[int]            # per clip the number of expanded columns
    sets: List[List[List[int]]]     # sets[b][n] = position n's class ids, the sheet's own first


def _readings_of(alternatives, label_lists: List[List[int]], keep_empty: bool = False) -> Optional[Readings]:
    """alternatives[b] = [(n, [class, ...]), ...]: label n of utterance b may also be sung as one of these classes -> Readings, or None when
    alternatives is None or all-empty (keep_empty: the Readings of a sheet without extras instead).  The lattice id of a position is its
    class id where it has no extras and READING_SET_ID + k for the k-th distinct multi-reading set of the clip (sets compared as sets),
    so that the equal-neighbour rule and the span rule see "the same label" exactly where the reading sets are equal; without extras the
    ids are the labels.  ValueError for a wrong list count, n outside 0 .. L_b-1, two entries for one n, an empty extras list, a class
    repeated within a set (the sheet's own included) or more than MAX_READINGS readings; NotImplementedError when a clip's expanded
    columns exceed MAX_READING_COLUMNS.  Host only."""
    if alternatives is None:
        return None
    if len(alternatives) != len(label_lists):
        raise ValueError(f"alternatives: {len(label_lists)} lists expected, one per utterance")
    sets, any_extra = [], False
    for b, labs in enumerate(label_lists):
        row = [[int(c)] for c in labs]
        seen = set()
        for n, extras in (alternatives[b] or ()):
            if int(n) != n or not 0 <= int(n) < len(labs):
                raise ValueError(f"alternatives[{b}]: position {n} outside 0..{len(labs) - 1}")
            n = int(n)
            if n in seen:
                raise ValueError(f"alternatives[{b}]: two entries for position {n}")
            seen.add(n)
            extras = [int(c) for c in extras]
            if not extras:
                raise ValueError(f"alternatives[{b}]: position {n} has an empty list of extra readings")
            row[n] = row[n] + extras
            if len(set(row[n])) != len(row[n]):
                raise ValueError(f"alternatives[{b}]: position {n} names a class twice (the sheet's own class {row[n][0]} included)")
            if len(row[n]) > MAX_READINGS:
                raise ValueError(f"alternatives[{b}]: position {n} has {len(row[n])} readings, at most {MAX_READINGS}")
            any_extra = True
        if sum(len(r) for r in row) > MAX_READING_COLUMNS:
            raise NotImplementedError(f"alternatives[{b}]: {sum(len(r) for r in row)} expanded columns exceed {MAX_READING_COLUMNS}")
        sets.append(row)
    if not any_extra and not keep_empty:
        return None
    B = len(label_lists)
    Lmax = max(1, max((len(l) for l in label_lists), default=1))
    n_columns = [sum(len(r) for r in row) for row in sets]
    labels_x = torch.zeros((B, max(1, max(n_columns, default=1))), dtype=torch.int32)
    alt_start = torch.zeros((B, Lmax + 1), dtype=torch.int32)
    lattice_ids = torch.zeros((B, Lmax), dtype=torch.int32)
    for b, row in enumerate(sets):
        flat = [c for r in row for c in r]
        if flat:
            labels_x[b, : len(flat)] = torch.tensor(flat, dtype=torch.int32)
        starts, known = [0], {}
        for r in row:
            starts.append(starts[-1] + len(r))
        alt_start[b] = torch.tensor(starts + [starts[-1]] * (Lmax + 1 - len(starts)), dtype=torch.int32)
        ids = [r[0] if len(r) == 1 else READING_SET_ID + known.setdefault(frozenset(r), len(known)) for r in row]
        if ids:
            lattice_ids[b, : len(ids)] = torch.tensor(ids, dtype=torch.int32)
    return Readings(labels_x, alt_start, lattice_ids, n_columns, sets)


def _readings_from_scores(reading, col_score, rd: Readings):
    """Device outputs of ops.reading_scores -> readings[b][n] = (class id of the reading with the largest segment score, [score per
    reading, the sheet's own class first]), or None for a skipped character."""
    pick, score, alt = reading.cpu().numpy(), col_score.cpu().numpy(), rd.alt_start.numpy()
    return [[None if pick[b, n] < 0 else (int(r[pick[b, n]]), [float(v) for v in score[b, alt[b, n]: alt[b, n + 1]]])
             for n, r in enumerate(row)] for b, row in enumerate(rd.sets)]


class ReadingRoute(NamedTuple):
    """The device side of one call with pronunciation alternatives (readings_route): the expanded emissions stay for the scores."""
    rd: Readings
    em_x: torch.Tensor
    alt_start: torch.Tensor
    em: torch.Tensor                # the folded matrix: run_lattice's input, with lattice_ids in the labels' place
    lattice_ids: torch.Tensor

    def scores(self, n_lab, onset, offset):
        """-> reading [B, Lmax] int32, col_score [B, columns] float64 (ops.reading_scores on the DP's boundaries)."""
        return ops.reading_scores(self.em_x, self.alt_start, n_lab, onset, offset)


def readings_route(rd: Readings, emissions_of, n_lab, nf, device) -> ReadingRoute:
    """The one route every caller takes: emissions_of(labels_x, n_columns) -- the existing head or prep, run on the expanded labels (device
    int32 tensors) -> the expanded compact matrix; ops.merge_readings folds it for the lattice."""
    em_x = emissions_of(rd.labels_x.to(device), torch.tensor(rd.n_columns, dtype=torch.int32).to(device))
    alt = rd.alt_start.to(device)
    return ReadingRoute(rd, em_x, alt, ops.merge_readings(em_x, alt, n_lab, nf), rd.lattice_ids.to(device))


OFF_SHEET_ID = 1 << 25          # lattice id of every off-sheet slot: no class id and no READING_SET_ID + k can equal it
OFF_SHEET_MAX_LABELS = 4095     # expanded labels per clip (sheet + slots): what the lattice takes
DEFAULT_OFF_SHEET_PENALTY = math.log(100.0)     # nats per frame: a 1 % share (NOT tuned on real singing)


class OffSheet(NamedTuple):
    """_off_sheet_of's result (host): the sheet with its off-sheet slots, in EXPANDED positions (a slot before label n sits in front of it),
    and the caller's keywords remapped to them.  optional_spans lists the caller's spans first, then one one-label span per slot."""
    slots: List[List[int]]          # the caller's positions n (0 .. L_b), ascending
    penalty: float
    label_lists: List[List[int]]    # expanded label rows: class 0 at a slot (the head and the prep write the floor there)
    lattice_ids: torch.Tensor       # [B, L'max] int32: the labels, OFF_SHEET_ID at a slot
    slot_cols: torch.Tensor         # [B, Fmax] int32: the slots' expanded positions, ascending (padding -1)
    n_slots: torch.Tensor           # [B] int32
    keep: List[List[int]]           # keep[b][n] = expanded position of the caller's label n
    optional_spans: list
    repeat_spans: Optional[list]
    char_windows: Optional[list]
    onset_anchors: Optional[list]
    alternatives: Optional[list]
    n_caller_spans: List[int]       # how many of optional_spans[b] are the caller's

    def slot_sets(self):
        return [set(int(q) for q in self.slot_cols[b, : len(s)].tolist()) for b, s in enumerate(self.slots)]

    def ids_with_slots(self, ids: torch.Tensor) -> torch.Tensor:
        """Host lattice ids [B, L'max] of the expanded rows (_readings_of's) with OFF_SHEET_ID at the slots."""
        ids = ids.clone()
        for b, s in enumerate(self.slots):
            if s:
                ids[b, self.slot_cols[b, : len(s)].long()] = OFF_SHEET_ID
        return ids


def _off_sheet_of(who: str, off_sheet, penalty, label_lists: List[List[int]], optional_spans=None, repeat_spans=None, char_windows=None,
                  onset_anchors=None, alternatives=None, narrow: bool = False) -> Optional[OffSheet]:
    """off_sheet[b] = [n, ...]: a slot BEFORE label n of utterance b, 0 <= n <= L_b (L_b = after the last label) -> OffSheet, or None when
    off_sheet is None or all-empty (the call as it was).  A slot is a label position of its own: with F slots the lattice has L' = L + F
    labels, label n at position n + #{slots <= n}.  Each slot gets a one-label optional span.  The caller's keywords move with the labels:
    an optional or repeat span (a, e) becomes (pos(a), pos(e-1) + 1) -- a slot strictly inside it belongs to it, one at either edge stays
    outside, so no slot span shares an end (a start) with it --; char_windows / onset_anchors / alternatives get pos(n).  An index the
    keyword's own check would refuse stays refusable (it is shifted, never clamped).
    ValueError for a wrong list count, an n that is no integer or outside 0 .. L_b, a duplicate, a slot on an utterance without labels, a
    negative or NaN penalty; NotImplementedError when L' exceeds OFF_SHEET_MAX_LABELS (narrow: POSTERIOR_MAX_LABELS, the confidences
    that stop there).  Host only."""
    if off_sheet is None:
        return None
    B = len(label_lists)
    if len(off_sheet) != B:
        raise ValueError(f"{who}: off_sheet: {B} lists expected, one per utterance")
    slots = []
    for b, given in enumerate(off_sheet):
        L, row = len(label_lists[b]), []
        for n in (() if given is None else given):         # a list, an array or a tensor row
            try:
                whole = not isinstance(n, bool) and bool(int(n) == n) and 0 <= int(n) <= L
            except (TypeError, ValueError, OverflowError):  # None, a string, NaN, inf
                whole = False
            if not whole:
                raise ValueError(f"{who}: off_sheet[{b}]: position {n} is not an integer in 0..{L}")
            row.append(int(n))
        if len(set(row)) != len(row):
            raise ValueError(f"{who}: off_sheet[{b}]: a position is named twice")
        if row and L == 0:
            raise ValueError(f"{who}: off_sheet[{b}]: a slot on an utterance without labels")
        slots.append(sorted(row))
    if not any(slots):
        return None
    penalty = float(penalty)
    if not penalty >= 0.0:
        raise ValueError(f"{who}: off_sheet_penalty must be >= 0 (nats per frame), not {penalty}")
    limit = POSTERIOR_MAX_LABELS if narrow else OFF_SHEET_MAX_LABELS
    for b, s in enumerate(slots):
        if len(label_lists[b]) + len(s) > limit:
            raise NotImplementedError(f"{who}: off_sheet[{b}]: {len(label_lists[b])} labels + {len(s)} slots exceed {limit}"
                                      + (" (the limit of this kind of confidence)" if narrow else ""))

    def pos(b, n):                    # expanded position of label n: every slot before label <= n lies in front of it
        return n + sum(1 for s in slots[b] if s <= n)

    def per_clip(given, move):
        if given is None:
            return None
        if len(given) != B:           # the keyword's own check refuses it
            return given
        return [[move(b, item) for item in (given[b] or ())] for b in range(B)]

    span = lambda b, ae: (pos(b, ae[0]), pos(b, ae[1] - 1) + 1)
    first = lambda b, item: (pos(b, item[0]), *item[1:])
    lists, keep, cols = [], [], torch.full((B, max(len(s) for s in slots)), -1, dtype=torch.int32)
    Lx = max(1, max(len(l) + len(s) for l, s in zip(label_lists, slots)))
    ids = torch.zeros((B, Lx), dtype=torch.int32)
    for b, labs in enumerate(label_lists):
        row = [0] * (len(labs) + len(slots[b]))
        keep.append([pos(b, n) for n in range(len(labs))])
        for n, c in enumerate(labs):
            row[keep[b][n]] = int(c)
        lists.append(row)
        if row:
            ids[b, : len(row)] = torch.tensor(row, dtype=torch.int32)
        for i, s in enumerate(slots[b]):
            cols[b, i] = s + i
            ids[b, s + i] = OFF_SHEET_ID
    own = per_clip(optional_spans, span)
    if own is not None and len(own) != B:         # the keyword's own check refuses it
        spans, n_own = own, [0] * B
    else:
        own = own if own is not None else [[] for _ in range(B)]
        n_own = [len(v) for v in own]
        spans = [list(own[b]) + [(q, q + 1) for q in cols[b, : len(slots[b])].tolist()] for b in range(B)]
    return OffSheet(slots, penalty, lists, ids, cols, torch.tensor([len(s) for s in slots], dtype=torch.int32), keep, spans,
                    per_clip(repeat_spans, span), per_clip(char_windows, first), per_clip(onset_anchors, first),
                    per_clip(alternatives, first), n_own)


def _off_sheet_visits(off: OffSheet, r, frame_counts):
    """The slot visits of a lattice result -> per clip the time-ordered list of (n, first frame, last frame + 1): from the path where the
    lattice has one (a slot under a repeat span may be visited several times), else from the slot positions' onset / offset."""
    out = []
    rows = None if r.path is None else r.path.cpu().numpy()
    on, offs = r.onset.cpu().numpy(), r.offset.cpu().numpy()
    for b, s in enumerate(off.slots):
        at = {int(q): n for q, n in zip(off.slot_cols[b, : len(s)].tolist(), s)}
        if rows is not None:
            out.append([(at[p], t, u) for p, t, u in _visits_of_row(rows[b, : int(frame_counts[b])]) if p in at])
        else:
            out.append(sorted(((n, int(on[b, q]), int(offs[b, q])) for q, n in at.items() if on[b, q] >= 0), key=lambda v: v[1]))
    return out


def _off_sheet_top(off: OffSheet, visits, em_c, pron: "Pronunciation", device):
    """What was heard in every slot visit: ops.segment_class_scores over the visits' frames (no own class) -> per clip, per visit the list
    [(class id, score per frame), ...]."""
    V = max(1, max(len(v) for v in visits))
    on = torch.full((len(visits), V), -1, dtype=torch.int32)
    offs = torch.full((len(visits), V), -1, dtype=torch.int32)
    for b, vis in enumerate(visits):
        for i, (_, t, u) in enumerate(vis):
            on[b, i], offs[b, i] = t, u
    n_vis = torch.tensor([len(v) for v in visits], dtype=torch.int32).to(device)
    top_col, top_score, _, _, n_seg = (t.cpu().numpy() for t in ops.segment_class_scores(
        em_c, n_vis, on.to(device), offs.to(device), torch.full((len(visits), V), -1, dtype=torch.int32).to(device), pron.top_k))
    return [[[(pron.classes[j], float(s) / max(int(n_seg[b, i]), 1)) for j, s in zip(top_col[b, i], top_score[b, i]) if j >= 0]
             for i in range(len(vis))] for b, vis in enumerate(visits)]


def _without_slots(off: OffSheet, b: int, row):
    return [row[p] for p in off.keep[b]]


def _scores_without_slots(off: OffSheet, scores, segments_x=None):
    """The score dicts of the expanded lattice -> the caller's: per-character lists lose the slot entries, span_skip_prob keeps the
    caller's spans, repeat_count goes back to the caller's (a, e) key by key (a span begins and ends on labels), visit_occupancy loses the slot visits (segments_x: the expanded
    segments it is parallel to) and "off_sheet_prob" {n: sung_prob / visits of the slot} is added where the dict has that number."""
    slot_sets = off.slot_sets()
    for b, d in enumerate(scores):
        per_char = d.get("sung_prob", d.get("visits"))
        if per_char is not None:
            d["off_sheet_prob"] = {n: per_char[int(q)] for n, q in zip(off.slots[b], off.slot_cols[b].tolist())}
        for key in ("occupancy", "onset_prob", "offset_prob", "sung_prob", "visits"):
            if key in d:
                d[key] = _without_slots(off, b, d[key])
        if "span_skip_prob" in d:
            d["span_skip_prob"] = d["span_skip_prob"][: off.n_caller_spans[b]]
        if "repeat_count" in d:
            back = {p: n for n, p in enumerate(off.keep[b])}          # expanded position -> the caller's label
            d["repeat_count"] = {(back[a], back[e - 1] + 1): v for (a, e), v in d["repeat_count"].items()}
        if "visit_occupancy" in d and segments_x is not None:
            d["visit_occupancy"] = [v for v, seg in zip(d["visit_occupancy"], segments_x[b]) if seg[0] not in slot_sets[b]]
    return scores


def _segments_without_slots(off: OffSheet, segments_x):
    back = [{p: n for n, p in enumerate(k)} for k in off.keep]
    return [[(back[b][p], t, u) for p, t, u in segs if p in back[b]] for b, segs in enumerate(segments_x)]


MAX_PRONUNCIATION_COLUMNS = 4095      # label columns (the sheet's, or the expanded readings') plus candidate classes: what the head / prep take


class Pronunciation(NamedTuple):
    """_pronunciation_of's result (host): what the route with pronunciation scores needs beside the labels."""
    classes: List[int]              # the candidate class ids, sorted and unique: candidate column j holds classes[j]
    top_k: int
    own_col: torch.Tensor           # [B, Lmax] int32: the candidate column of the sheet's class per position, -1 beyond a clip's labels
    col_of: torch.Tensor            # [largest class id + 1] int32: class id -> candidate column, -1 = not a candidate


def _pronunciation_of(who: str, return_pronunciation, pronunciation_classes, pronunciation_top_k, label_lists: List[List[int]],
                      rd: Optional[Readings] = None, slots=None) -> Optional[Pronunciation]:
    """The three keywords of the pronunciation scores -> Pronunciation, or None when return_pronunciation is off (the call as it was).
    pronunciation_classes: an int N (classes 1 .. N) or a sequence of class ids; the sheet's own classes (with alternatives: every
    reading's) are unioned in; sorted and unique.  ValueError for a missing class list, an id below 1 or a top_k outside 1 .. 16;
    NotImplementedError when the label columns (rd: the widest expanded row) plus the candidates exceed MAX_PRONUNCIATION_COLUMNS.
    slots (OffSheet.slot_sets(), or None): label positions that are off-sheet slots -- the union ignores them and own_col is -1 there.
    Host only."""
    if not return_pronunciation:
        return None
    if pronunciation_classes is None:
        raise ValueError(f"{who}: return_pronunciation needs pronunciation_classes (an int N for classes 1..N, or a sequence of class ids)")
    if isinstance(pronunciation_top_k, bool) or int(pronunciation_top_k) != pronunciation_top_k \
            or not 1 <= int(pronunciation_top_k) <= ops.MAX_PRONUNCIATION_TOP_K:
        raise ValueError(f"{who}: pronunciation_top_k must be an int in 1..{ops.MAX_PRONUNCIATION_TOP_K}")
    if isinstance(pronunciation_classes, bool):
        raise ValueError(f"{who}: pronunciation_classes must be an int N (classes 1..N) or a sequence of class ids")
    if isinstance(pronunciation_classes, (int, np.integer)):
        if pronunciation_classes < 1:
            raise ValueError(f"{who}: pronunciation_classes = {pronunciation_classes}: at least class 1 expected")
        given = range(1, int(pronunciation_classes) + 1)
    else:
        given = [int(c) for c in pronunciation_classes]
        if any(c < 1 for c in given):
            raise ValueError(f"{who}: pronunciation_classes: class ids start at 1")
    rows = rd.sets if rd is not None else [[[int(c)] for c in row] for row in label_lists]
    sheet = [c for b, row in enumerate(rows) for n, r in enumerate(row) for c in r if slots is None or n not in slots[b]]
    classes = sorted(set(given) | set(sheet))
    Lmax = max(1, max((len(l) for l in label_lists), default=1))
    width = rd.labels_x.shape[1] if rd is not None else Lmax
    if width + len(classes) > MAX_PRONUNCIATION_COLUMNS:
        raise NotImplementedError(f"{who}: {width} label columns + {len(classes)} pronunciation classes exceed {MAX_PRONUNCIATION_COLUMNS}")
    col_of = torch.full((classes[-1] + 1,), -1, dtype=torch.int32)
    col_of[torch.tensor(classes, dtype=torch.int64)] = torch.arange(len(classes), dtype=torch.int32)
    own_col = torch.full((len(label_lists), Lmax), -1, dtype=torch.int32)
    for b, row in enumerate(label_lists):
        if row:
            own_col[b, : len(row)] = col_of[torch.tensor(row, dtype=torch.int64)]
        for n in (slots[b] if slots is not None else ()):
            own_col[b, n] = -1
    return Pronunciation(classes, int(pronunciation_top_k), own_col, col_of)


def _widened_labels(lab: torch.Tensor, n: torch.Tensor, classes: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Label rows lab [B, W] / counts n [B] and the candidate classes [C] (int32, one device) -> the rows the head or the prep is asked
    for: lab's rows, their padding filled with a valid class (classes[0]; those columns are never read), then the C candidates at the
    fixed columns W .. W + C - 1, and the count W + C for every clip."""
    W = lab.shape[1]
    own = torch.where(torch.arange(W, device=lab.device)[None, :] < n[:, None], lab, classes[0])
    lab_w = torch.cat([own, classes[None, :].expand(lab.shape[0], -1)], dim=1).contiguous()
    return lab_w, torch.full_like(n, W + classes.shape[0])


def _own_columns(pron: Pronunciation, route, reading, device) -> torch.Tensor:
    """own_col [B, Lmax] int32 on the device: the sheet's class per position, or with alternatives (route) the reading that
    ops.reading_scores picked (`reading`), gathered on the device; -1 for a skipped position and beyond a clip's labels."""
    if route is None:
        return pron.own_col.to(device)
    Lmax = reading.shape[1]
    at = (route.alt_start[:, :Lmax] + reading.clamp(min=0)).clamp(max=route.rd.labels_x.shape[1] - 1).long()
    picked = torch.gather(route.rd.labels_x.to(device), 1, at).long()
    valid = (reading >= 0) & (pron.own_col.to(device) >= 0)
    return torch.where(valid, pron.col_of.to(device)[picked.clamp(max=pron.col_of.shape[0] - 1)], torch.full_like(reading, -1))


def _pronunciation_from_scores(scores, own_col, pron: Pronunciation, label_lists):
    """Device outputs of ops.segment_class_scores -> pronunciation[b][n] = None for a skipped character, else {"class": the own class id,
    "frames": n, "log_prob": own_score / n, "rank": own_rank, "gop": (own_score - top_score[0]) / n, "top": [(class id, score / n),
    ...]}.  gop <= 0, and 0.0 where the own class has the best sum (stated without the subtraction: -inf beside -inf)."""
    top_col, top_score, own_score, own_rank, n_seg = (t.cpu().numpy() for t in scores[:5])
    own = own_col.cpu().numpy()
    out = []
    for b, labs in enumerate(label_lists):
        row = []
        for n in range(len(labs)):
            if top_col[b, n, 0] < 0:
                row.append(None)
                continue
            frames, mine, best = int(n_seg[b, n]), float(own_score[b, n]), float(top_score[b, n, 0])
            per = max(frames, 1)
            row.append({"class": pron.classes[own[b, n]] if own[b, n] >= 0 else int(labs[n]), "frames": frames, "log_prob": mine / per,
                        "rank": int(own_rank[b, n]), "gop": 0.0 if mine == best else (mine - best) / per,
                        "top": [(pron.classes[j], float(s) / per) for j, s in zip(top_col[b, n], top_score[b, n]) if j >= 0]})
        out.append(row)
    return out


def _visits_of_row(row):
    """One clip's lattice state per frame -> the time-ordered list of (char_index, first frame, last frame + 1) of every visit: the maximal
    runs of frames in one odd lattice state."""
    visits, t = [], 0
    while t < len(row):
        u = t
        while u + 1 < len(row) and row[u + 1] == row[t]:
            u += 1
        if row[t] >= 0 and row[t] % 2 == 1:
            visits.append((int(row[t]) // 2, t, u + 1))
        t = u + 1
    return visits


def _segments_from_path(path, frame_counts: Sequence[int], hop_size_second: float):
    """path [B, T] (ops.viterbi_repeats_batch) -> per utterance the time-ordered list of (char_index, onset_s, offset_s) of every visit: the
    maximal runs of frames in one odd lattice state (a repeated line has one visit per time it was sung)."""
    rows = path.cpu().numpy()
    return [[(n, float(t) * hop_size_second, float(u) * hop_size_second) for n, t, u in _visits_of_row(rows[b, : int(T)])]
            for b, T in enumerate(frame_counts)]


def _frame_bound(seconds: float, hop: float, n_frames: int, up: bool) -> int:
    """ceil (up) or floor of seconds / hop with a 1e-9 guard against the division's rounding, clamped to -1 .. n_frames + 1."""
    x = min(max(float(seconds) / hop, -1.0), float(n_frames) + 1.0)
    return int(math.ceil(x - 1e-9)) if up else int(math.floor(x + 1e-9))


def windows_from_anchors(n_labels: int, n_frames: int, char_windows=None, onset_anchors=None,
                         hop_size_second: float = 0.02) -> Tuple[List[int], List[int]]:
    """One clip's per-state frame windows (include/lyricalign.h la_viterbi_windows_batch) from what is known about time: -> (lo, hi), two
    lists of 2 * n_labels + 1 ints; state s (0 = leading silence, 2n+1 = character n, 2n+2 = the silence after it) may hold the path at
    frame t only if lo[s] <= t < hi[s].  Without constraints every window is [0, n_frames).  Host only.
    char_windows = [(n, lo_s, hi_s), ...]: character n's segment lies inside [lo_s, hi_s] seconds (either side None = open): state 2n+1
    gets lo = ceil(lo_s / hop), hi = floor(hi_s / hop) (exclusive, as the reported offset is the last frame + 1).
    onset_anchors = [(n, t_s, tol_s), ...]: if character n is on the path its onset lies within tol_s of t_s.  With [f_lo, f_hi] the
    frames f with |f * hop - t_s| <= tol_s, widened to hold round(t_s / hop): state 2n+1 gets lo = f_lo and EVERY state below 2n+1 gets
    hi = f_hi, so that the path has reached state 2n+1 (or passed it) by frame f_hi -- the bound a window on the character alone cannot
    give, as the silence before it could stretch past it.
    Several constraints on one state intersect.  ValueError for an index outside 0 .. n_labels-1, a negative tolerance, or a NaN."""
    L, T, hop = int(n_labels), int(n_frames), float(hop_size_second)
    if L < 0 or T < 0 or not hop > 0.0:
        raise ValueError("windows_from_anchors: n_labels >= 0, n_frames >= 0 and hop_size_second > 0 expected")
    lo, hi = [0] * (2 * L + 1), [T] * (2 * L + 1)

    def index(n, what):
        if isinstance(n, float) and n != n:
            raise ValueError(f"windows_from_anchors: {what}: NaN")
        if int(n) != n or not 0 <= int(n) < L:
            raise ValueError(f"windows_from_anchors: {what}: character index {n} outside 0..{L - 1}")
        return int(n)

    def number(v, what):
        v = float(v)
        if v != v:
            raise ValueError(f"windows_from_anchors: {what}: NaN")
        return v

    for n, lo_s, hi_s in (char_windows or ()):
        s = 2 * index(n, "char_windows") + 1
        if lo_s is not None:
            lo[s] = max(lo[s], _frame_bound(number(lo_s, "char_windows"), hop, T, True))
        if hi_s is not None:
            hi[s] = min(hi[s], _frame_bound(number(hi_s, "char_windows"), hop, T, False))
    for n, t_s, tol_s in (onset_anchors or ()):
        s = 2 * index(n, "onset_anchors") + 1
        t_s, tol_s = number(t_s, "onset_anchors"), number(tol_s, "onset_anchors")
        if tol_s < 0.0:
            raise ValueError(f"windows_from_anchors: onset_anchors: negative tolerance {tol_s}")
        nearest = int(math.floor(min(max(t_s / hop, -1.0), T + 1.0) + 0.5))
        f_lo = min(_frame_bound(t_s - tol_s, hop, T, True), nearest)
        f_hi = max(_frame_bound(t_s + tol_s, hop, T, False), nearest)
        lo[s] = max(lo[s], f_lo)
        for below in range(s):
            hi[below] = min(hi[below], f_hi)
    return lo, hi


def _windows_of(char_windows, onset_anchors, label_lists: List[List[int]], frame_counts: Sequence[int], hop_size_second: float):
    """char_windows / onset_anchors: per utterance a list in windows_from_anchors' form (or None) -> host int32 tensors (win_lo, win_hi)
    [B, 2 * Lmax + 1] in each utterance's own frames, or None when no utterance has a constraint (None or all-empty keywords)."""
    B = len(label_lists)
    for name, per in (("char_windows", char_windows), ("onset_anchors", onset_anchors)):
        if per is not None and len(per) != B:
            raise ValueError(f"{name}: {B} lists expected, one per utterance")
    if not any(per is not None and any(len(v or ()) for v in per) for per in (char_windows, onset_anchors)):
        return None
    Lmax = max(1, max((len(l) for l in label_lists), default=1))
    win_lo = torch.zeros((B, 2 * Lmax + 1), dtype=torch.int32)
    win_hi = torch.zeros((B, 2 * Lmax + 1), dtype=torch.int32)
    for b, labs in enumerate(label_lists):
        lo, hi = windows_from_anchors(len(labs), int(frame_counts[b]), char_windows[b] if char_windows is not None else None,
                                      onset_anchors[b] if onset_anchors is not None else None, hop_size_second)
        win_lo[b, : len(lo)] = torch.tensor(lo, dtype=torch.int32)
        win_hi[b, : len(hi)] = torch.tensor(hi, dtype=torch.int32)
    return win_lo, win_hi


def _seconds_from_frames(onset, offset, status, label_lists, hop_size_second, skipped_as_none: bool = False):
    """skipped_as_none (the span lattice): a label with onset -1 under LA_OK was inside a taken jump -> None in place of [onset, offset]."""
    on, off, st = onset.cpu().numpy(), offset.cpu().numpy(), status.cpu().numpy()
    result = []
    for b, labs in enumerate(label_lists):
        if st[b] == LA_EEMPTY:
            raise IndexError("index 0 is out of bounds for axis 0 with size 0")          # (:152)
        if st[b] == LA_EINFEASIBLE:
            k = int(np.argmax(on[b, : len(labs)] < 0)) * 2 + 1
            raise ValueError(f"{k} is not in list")                                         # (:183)
        if st[b] != LA_OK:
            raise _lib.LyricAlignHipError(f"viterbi status {int(st[b])} for utterance {b}")
        result.append([None if (skipped_as_none and on[b, n] < 0) else
                       [float(int(on[b, n])) * hop_size_second, float(int(off[b, n])) * hop_size_second]
                       for n in range(len(labs))])                                         # (:185) float(frame) * hop
    return result


def _scores_from_posteriors(occupancy, onset_prob, offset_prob, log_z, final_score, label_lists, present_prob=None, span_skip_prob=None,
                            optional_spans=None, log_z_free=None):
    """Device outputs of ops.alignment_posteriors -> per-utterance dicts of Python floats (after _seconds_from_frames
    has raised for failed utterances).  path_log_posterior = final_score - log_z <= 0: log-probability of the reported path.
    With present_prob / span_skip_prob (ops.alignment_posteriors_spans) each dict also holds "sung_prob": [L] and "span_skip_prob":
    one value per span of optional_spans[b], in the order given.  With log_z_free (the same lattice without frame windows) also
    "window_log_prob" = log_z - log_z_free <= 0: the log-probability the unanchored model gives to "the path lies inside the windows"."""
    occ, onp, offp = occupancy.cpu().numpy(), onset_prob.cpu().numpy(), offset_prob.cpu().numpy()
    lz, fs = log_z.cpu().numpy(), final_score.cpu().numpy()
    out = [{"occupancy": [float(v) for v in occ[b, : len(labs)]],
            "onset_prob": [float(v) for v in onp[b, : len(labs)]],
            "offset_prob": [float(v) for v in offp[b, : len(labs)]],
            "path_log_posterior": float(fs[b] - lz[b])} for b, labs in enumerate(label_lists)]
    if present_prob is not None:
        pres, skp = present_prob.cpu().numpy(), span_skip_prob.cpu().numpy()
        for b, labs in enumerate(label_lists):
            out[b]["sung_prob"] = [float(v) for v in pres[b, : len(labs)]]
            out[b]["span_skip_prob"] = [float(skp[b, int(n)]) for _, n in ((optional_spans[b] or ()) if optional_spans is not None else ())]
    if log_z_free is not None:
        lzf = log_z_free.cpu().numpy()
        for b in range(len(label_lists)):
            out[b]["window_log_prob"] = float(lz[b] - lzf[b])
    return out


class LatticeResult(NamedTuple):
    """Device tensors of one run_lattice call, in the order of AlignModel.align(return_frames=True); what was not asked for is None."""
    onset: torch.Tensor
    offset: torch.Tensor
    score: torch.Tensor
    status: torch.Tensor
    occupancy: Optional[torch.Tensor] = None
    onset_prob: Optional[torch.Tensor] = None
    offset_prob: Optional[torch.Tensor] = None
    log_z: Optional[torch.Tensor] = None
    present_prob: Optional[torch.Tensor] = None
    span_skip_prob: Optional[torch.Tensor] = None
    log_z_free: Optional[torch.Tensor] = None
    # behind the eleven tuple fields, as plain attributes (None where they do not apply; run_lattice's _result sets them)
    path = None             # [B, T] int32, the lattice state per frame: ops.viterbi_repeats_batch's fifth output
    visits = None           # [B, Lmax] (= present_prob, an expected count), repeat_count [B, Lmax], path_prob [B, T]: the repeat sweeps'
    repeat_count = None
    path_prob = None
    in_order = None         # [B, Lmax]: the line-order sweep's (ops.alignment_posteriors_lines), with `visits` and `path_prob`


class RepeatLatticeResult(LatticeResult):
    """LatticeResult of the lattice with repeatable spans: the same eleven tuple fields (seven are None unless confidence="repeat" was
    asked for; present_prob then holds `visits`, an expected count) and, behind them as attributes, `path` [B, T] int32 -- the lattice
    state per frame, ops.viterbi_repeats_batch's fifth output -- and with confidence="repeat" `visits` [B, Lmax] (= present_prob),
    `repeat_count` [B, Lmax] and `path_prob` [B, T] (ops.alignment_posteriors_repeats)."""


def _result(dp, post=(), log_z_free=None) -> LatticeResult:
    """A DP entry's tuple, a sweep's (or none) and log_z_free -> the LatticeResult; a DP with a path (ops.viterbi_repeats_batch) gives a
    RepeatLatticeResult with the path and the repeat sweep's further outputs as attributes."""
    fields = (*dp[:4], *post[:4], *post[5:7])
    if len(dp) == 4:
        return LatticeResult(*fields, log_z_free=log_z_free)
    r = RepeatLatticeResult(*fields, log_z_free=log_z_free)
    r.path, r.visits = dp[4], r.present_prob
    r.repeat_count, r.path_prob = post[7:9] or (None, None)
    return r


POSTERIOR_MAX_LABELS = 511      # one lane per lattice state in the sum-product sweeps and in the span / window entries of the DP


class Route(NamedTuple):
    """One row of ROUTES: the ops entries behind one (confidence, spans given, windows given)."""
    dp: str
    posteriors: Optional[str] = None
    free: Optional[str] = None      # log_z_free: None, "log_z" (the sweep's own) or [3] of one more call of this entry without windows


# THE dispatch table: (confidence, spans given, windows given) -> Route.  tests/test_gpu_lattice_dispatch.py restates eleven of its rows.
# ("plain" is meant for the lattice without spans and windows and "span" for the one without windows; their other rows say what such a
# call has always made.  A "span" row with windows sweeps once more for a log_z_free that its result does not hold.)
ROUTES = {
    (None, False, False): Route("viterbi_batch"),
    (None, True, False): Route("viterbi_spans_batch"),
    (None, False, True): Route("viterbi_windows_batch"),
    (None, True, True): Route("viterbi_windows_batch"),
    ("plain", False, False): Route("viterbi_batch", "alignment_posteriors"),
    ("plain", True, False): Route("viterbi_spans_batch", "alignment_posteriors"),
    ("plain", False, True): Route("viterbi_windows_batch", "alignment_posteriors"),
    ("plain", True, True): Route("viterbi_windows_batch", "alignment_posteriors"),
    ("span", False, False): Route("viterbi_batch", "alignment_posteriors_spans"),
    ("span", True, False): Route("viterbi_spans_batch", "alignment_posteriors_spans"),
    ("span", False, True): Route("viterbi_windows_batch", "alignment_posteriors_windows", "alignment_posteriors"),
    ("span", True, True): Route("viterbi_windows_batch", "alignment_posteriors_windows", "alignment_posteriors_spans"),
    ("anchored", False, False): Route("viterbi_batch", "alignment_posteriors_spans", "log_z"),
    ("anchored", True, False): Route("viterbi_spans_batch", "alignment_posteriors_spans", "log_z"),
    ("anchored", False, True): Route("viterbi_windows_batch", "alignment_posteriors_windows", "alignment_posteriors"),
    ("anchored", True, True): Route("viterbi_windows_batch", "alignment_posteriors_windows", "alignment_posteriors_spans"),
    ("sheet", False, False): Route("viterbi_batch", "alignment_posteriors_lattice", "log_z"),
    ("sheet", True, False): Route("viterbi_spans_batch", "alignment_posteriors_lattice", "log_z"),
    ("sheet", False, True): Route("viterbi_windows_batch", "alignment_posteriors_lattice", "alignment_posteriors_lattice"),
    ("sheet", True, True): Route("viterbi_windows_batch", "alignment_posteriors_lattice", "alignment_posteriors_lattice"),
    ("repeat", False, False): Route("viterbi_repeats_batch", "alignment_posteriors_repeats"),
    ("repeat", True, False): Route("viterbi_repeats_batch", "alignment_posteriors_repeats"),
    ("repeat", False, True): Route("viterbi_repeats_batch", "alignment_posteriors_repeats", "alignment_posteriors_repeats"),
    ("repeat", True, True): Route("viterbi_repeats_batch", "alignment_posteriors_repeats", "alignment_posteriors_repeats"),
    ("song", False, False): Route("viterbi_repeats_batch", "alignment_posteriors_song"),
    ("song", True, False): Route("viterbi_repeats_batch", "alignment_posteriors_song"),
    ("song", False, True): Route("viterbi_repeats_batch", "alignment_posteriors_song", "alignment_posteriors_song"),
    ("song", True, True): Route("viterbi_repeats_batch", "alignment_posteriors_song", "alignment_posteriors_song"),
}
# The rules that lie across the table.  A given repeat_from sends the DP to the lattice with repeatable spans (the rows of "repeat"
# and "song" name it themselves); beyond POSTERIOR_MAX_LABELS the DP's span and window entries give way to the general one.
REPEAT_DP = "viterbi_repeats_batch"
WIDE_DP = {"viterbi_spans_batch": "viterbi_lattice_batch", "viterbi_windows_batch": "viterbi_lattice_batch"}
# and a third: a given line_start sends the DP to the lattice with free line order, which knows none of the table's faces
LINES_DP = "viterbi_lines_batch"
LINES_SWEEP, LINES_CONFIDENCE = "alignment_posteriors_lines", "lines"       # and, for confidence="lines", its sum-product sweep behind it
# the sweeps of one lane per lattice state, and how run_lattice's refusal beyond POSTERIOR_MAX_LABELS ends for each
NARROW_SWEEPS = {name: "the posterior sweeps (the alignment itself and the sheet confidence take up to 4095)"
                 for name in ("alignment_posteriors", "alignment_posteriors_spans", "alignment_posteriors_windows")}
NARROW_SWEEPS["alignment_posteriors_repeats"] = "the posteriors on the lattice with repeatable spans"
# What an ops entry takes behind (em, labels, n_labels, n_frames [, onset, offset]), in its own order: "skip" = skip_from, skip_penalty;
# "win" = win_lo, win_hi; "repeat" = repeat_from, repeat_penalty; "path"; "bw" = boundary_window, which the entries that do not list it
# take by keyword.
ENTRY_ARGS = {
    "viterbi_batch": (), "viterbi_spans_batch": ("skip",), "viterbi_windows_batch": ("win", "skip"), "viterbi_lattice_batch": ("skip", "win"),
    "viterbi_repeats_batch": ("skip", "win", "repeat"),
    "alignment_posteriors": ("bw",), "alignment_posteriors_spans": ("skip", "bw"), "alignment_posteriors_windows": ("win", "skip", "bw"),
    "alignment_posteriors_lattice": ("skip", "win"), "alignment_posteriors_repeats": ("skip", "win", "repeat", "path"),
    "alignment_posteriors_song": ("skip", "win", "repeat", "path")}


def route_of(confidence, spans: bool, windows: bool, wide: bool = False, repeats: bool = False) -> Route:
    """ROUTES' row with the two rules applied: repeats = a repeat_from is given, wide = more than POSTERIOR_MAX_LABELS labels."""
    route = ROUTES[confidence, spans, windows]
    dp = REPEAT_DP if repeats else route.dp
    if wide:
        dp = WIDE_DP.get(dp, dp)
    return route if dp == route.dp else route._replace(dp=dp)


def _call(name: str, lattice, groups, boundary_window=None):
    """ops.<name> on lattice = (em, lab, n_lab, nf [, onset, offset]) with the argument groups that ENTRY_ARGS lists for it."""
    takes = ENTRY_ARGS[name]
    kw = {} if boundary_window is None or "bw" in takes else {"boundary_window": boundary_window}
    return getattr(ops, name)(*lattice, *(v for group in takes for v in groups[group]), **kw)


def run_lattice(em, lab, n_lab, nf, skip_from=None, windows=None, skip_penalty=0.0, confidence=None, boundary_window=2, dp=None,
                repeat_from=None, repeat_penalty=0.0, line_start=None, line_jump_penalty=0.0) -> LatticeResult:
    """The one place where the face of an alignment is decided (csrc/la_lattice.h Face, through the ops wrappers): the DP and, if asked
    for, the posteriors on the lattice that skip_from (host rows of _skip_from_of_spans, or None) and windows (host (win_lo, win_hi)
    of _windows_of, or None) describe.  em / lab / n_lab / nf are device tensors.
    confidence: None | "plain" (ops.alignment_posteriors; no spans, no windows) | "span" (the span lattice's; no windows; without a
    span the plain DP's frames, which are the span DP's bit for bit, and an all -1 skip_from) | "anchored" (posteriors GIVEN the windows,
    plus log_z_free = log_z of the same lattice without windows: one more launch of the free sweep, and log_z itself without windows).
    dp: the (onset, offset, score, status) of the plain lattice where they exist already (the fused head's).
    "sheet" (whole songs): any face at any size up to 4095 labels.  The DP runs by the routing below; the posteriors come from ONE call of
    ops.alignment_posteriors_lattice on the lattice given, log_z_free from a second call without windows where windows were given, else
    from log_z itself; the result is filled exactly as for "anchored".
    More than 511 labels (up to 4095): the DP with spans or windows is ops.viterbi_lattice_batch; the three older kinds of confidence
    stop at 511 and raise NotImplementedError before anything is launched ("sheet" is the kind for whole songs).
    repeat_from (host rows of _repeat_from_of_spans, or None) / repeat_penalty: the lattice with repeatable spans, at any size up to
    4095 labels, with or without skip_from and windows -- ops.viterbi_repeats_batch; the result's `path` holds the state per frame.  The
    four older kinds of confidence do not exist on that lattice: ValueError before anything is launched.
    "repeat": the posteriors of that lattice (ops.alignment_posteriors_repeats on the DP's onset / offset / path; repeat_from None = no
    repeat span), up to 511 labels (NotImplementedError before anything is launched).  The eleven fields are filled as for "sheet" with
    `visits` (an expected count) in present_prob's place -- log_z_free from a second sweep without windows where windows were given,
    None otherwise -- and repeat_count / path_prob are attributes of the result.
    "song": "repeat" without the label limit (whole songs, up to 4095 labels): ops.viterbi_repeats_batch, then ONE call of
    ops.alignment_posteriors_song, and a second one without windows for log_z_free where windows were given.  Up to 511 labels its
    numbers are "repeat"'s exactly.
    line_start (host rows of _line_start_of, or None) / line_jump_penalty: the lattice of an unmarked sheet, whose lines may be sung in any
    order (LINES_DP, ops.viterbi_lines_batch, up to 4095 labels); the result is a RepeatLatticeResult whose `path` holds the state per
    frame.  That lattice has the line breaks and nothing else: ValueError before anything is launched when line_start comes together
    with skip_from, windows, repeat_from or any of the six confidences above.
    "lines" (only with a line_start: ValueError without): the posteriors of that lattice -- LINES_DP, then ONE call of LINES_SWEEP
    (ops.alignment_posteriors_lines) on the DP's onset / offset / path.  occupancy, onset_prob, offset_prob and log_z are filled,
    present_prob holds `visits` (an expected count), and visits / in_order / path_prob are attributes of the result."""
    if confidence == LINES_CONFIDENCE and line_start is None:
        raise ValueError("run_lattice: confidence=\"lines\" is the posteriors of the lattice with free line order: it needs a line_start")
    if line_start is not None:
        for name, given in (("skip_from", skip_from), ("windows", windows), ("repeat_from", repeat_from),
                            ("confidence", None if confidence == LINES_CONFIDENCE else confidence)):
            if given is not None:
                raise ValueError(f"run_lattice: line_start does not go with {name} (the lattice with free line order has neither marked "
                                 "spans nor windows, and its posteriors are confidence=\"lines\")")
        rows = line_start.to(em.device)
        dp = getattr(ops, LINES_DP)(em, lab, n_lab, nf, rows, line_jump_penalty)
        r = _result(dp)
        if confidence is None:
            return r
        post = getattr(ops, LINES_SWEEP)(em, lab, n_lab, nf, dp[0], dp[1], rows, line_jump_penalty, dp[4], boundary_window)
        r = r._replace(occupancy=post[0], onset_prob=post[1], offset_prob=post[2], log_z=post[3], present_prob=post[5])
        r.path, r.visits, r.in_order, r.path_prob = dp[4], post[5], post[6], post[7]
        return r
    key = (confidence, skip_from is not None, windows is not None)
    if key not in ROUTES:
        raise ValueError(f"run_lattice: unknown confidence {confidence!r}")
    route = ROUTES[key]
    if repeat_from is not None and route.posteriors is not None and route.dp != REPEAT_DP:
        raise ValueError("run_lattice: on the lattice with repeatable spans the posteriors are confidence=\"repeat\" or \"song\" "
                         "(repeat_from does not go with the four older kinds)")
    wide = lab.shape[1] > POSTERIOR_MAX_LABELS
    if wide and route.posteriors in NARROW_SWEEPS:
        raise NotImplementedError(f"run_lattice: {lab.shape[1]} labels exceed the {POSTERIOR_MAX_LABELS}-label limit of "
                                  + NARROW_SWEEPS[route.posteriors])
    route = route_of(*key, wide, repeat_from is not None)
    dev = em.device
    skip_dev = None if skip_from is None else skip_from.to(dev)
    groups = {"skip": (skip_dev, skip_penalty), "win": (None, None) if windows is None else (windows[0].to(dev), windows[1].to(dev)),
              "repeat": (None if repeat_from is None else repeat_from.to(dev), repeat_penalty), "bw": (boundary_window,)}
    if dp is None or route.dp != "viterbi_batch":
        dp = _call(route.dp, (em, lab, n_lab, nf), groups)
    if route.posteriors is None:
        return _result(dp)
    groups["path"] = dp[4:5]
    if route.posteriors == "alignment_posteriors_spans" and skip_dev is None:          # the span entry wants its rows: none marked
        groups["skip"] = (torch.full((lab.shape[0], lab.shape[1] + 1), -1, dtype=torch.int32, device=dev), skip_penalty)
    frames = (em, lab, n_lab, nf, dp[0], dp[1])
    post = _call(route.posteriors, frames, groups, boundary_window)
    log_z_free = post[3] if route.free == "log_z" else None
    if route.free not in (None, "log_z"):
        log_z_free = _call(route.free, frames, {**groups, "win": (None, None), "path": (None,)}, boundary_window)[3]
    return _result(dp, post, None if confidence == "span" else log_z_free)


# A fourth rule beside REPEAT_DP, WIDE_DP and LINES_DP: given floors send the DP to the plain lattice with a minimum duration.  It has
# a function of its own beside run_lattice, whose parameter list is pinned: that lattice knows none of run_lattice's other arguments.
MIN_DURATION_DP = "viterbi_min_duration_batch"


def run_min_duration_lattice(em, lab, n_lab, nf, min_frames, skip_from=None, windows=None, confidence=None, repeat_from=None,
                             line_start=None) -> RepeatLatticeResult:
    """run_lattice's counterpart for the plain lattice with a floor under every character's duration: min_frames (host rows of
    _min_frames_of, never None here) -> MIN_DURATION_DP (ops.viterbi_min_duration_batch, up to 4095 labels) with the smallest chain depth
    that holds the rows' largest floor; the result is a RepeatLatticeResult whose `path` holds the state per frame.  The floor exists on
    the plain lattice alone and has no posteriors yet: ValueError before anything is launched when min_frames comes together with
    skip_from, windows, repeat_from, line_start or any confidence."""
    for name, given in (("skip_from", skip_from), ("windows", windows), ("repeat_from", repeat_from), ("line_start", line_start),
                        ("confidence", confidence)):
        if given is not None:
            raise ValueError(f"run_min_duration_lattice: min_frames does not go with {name} (the floor exists on the plain lattice alone, "
                             "and that lattice has no posteriors)")
    return _result(getattr(ops, MIN_DURATION_DP)(em, lab, n_lab, nf, min_frames.to(em.device), int(min_frames.max())))


def _formatted(r: LatticeResult, label_lists, hop_size_second, optional_spans):
    """What the public functions return for r: seconds, or (seconds, scores) when r holds posteriors.  The dicts of the span lattice
    (present_prob computed) name every span of optional_spans, or none where the caller gave no span.  A label with onset -1 under LA_OK
    was inside a taken jump (the lattice without spans has none) and comes back as None."""
    seconds = _seconds_from_frames(r.onset, r.offset, r.status, label_lists, hop_size_second, skipped_as_none=True)
    if r.occupancy is None:
        return seconds
    spans = None if r.present_prob is None else optional_spans if optional_spans is not None else [[] for _ in label_lists]
    return seconds, _scores_from_posteriors(r.occupancy, r.onset_prob, r.offset_prob, r.log_z, r.score, label_lists, r.present_prob,
                                            r.span_skip_prob, spans, r.log_z_free)


def _formatted_repeat(r: RepeatLatticeResult, label_lists, frame_counts, hop_size_second, optional_spans, repeat_spans):
    """What the public functions return for a run_lattice(confidence="repeat") result -> seconds, segments, scores.  scores[b] holds
    "occupancy", "onset_prob", "offset_prob" [L] (about the reported, FIRST visit), "path_log_posterior", "visits" [L] (the expected number
    of visits: it can exceed 1), "repeat_count" {(a, e): expected number of returns} for the spans of repeat_spans[b], "span_skip_prob"
    (one value per span of optional_spans[b]; an expected count under a repeat span), "visit_occupancy" (one number per entry of
    segments[b]: the mean posterior of the reported state over that visit's frames) and, where windows were given, "window_log_prob"."""
    seconds = _seconds_from_frames(r.onset, r.offset, r.status, label_lists, hop_size_second, skipped_as_none=True)
    spans = optional_spans if optional_spans is not None else [[] for _ in label_lists]
    scores = _scores_from_posteriors(r.occupancy, r.onset_prob, r.offset_prob, r.log_z, r.score, label_lists, r.visits, r.span_skip_prob,
                                     spans, r.log_z_free)
    rows, pp, rc = r.path.cpu().numpy(), r.path_prob.cpu().numpy(), r.repeat_count.cpu().numpy()
    segments = []
    for b, T in enumerate(frame_counts):
        visits = _visits_of_row(rows[b, : int(T)])
        segments.append([(n, float(t) * hop_size_second, float(u) * hop_size_second) for n, t, u in visits])
        d = scores[b]
        d["visits"] = d.pop("sung_prob")
        d["repeat_count"] = {(int(a), int(e)): float(rc[b, int(a)]) for a, e in ((repeat_spans[b] or ()) if repeat_spans is not None else ())}
        d["visit_occupancy"] = [float(pp[b, t:u].astype(np.float64).mean()) for _, t, u in visits]
    return seconds, segments, scores


def _formatted_lines(r: RepeatLatticeResult, label_lists, frame_counts, hop_size_second, line_start):
    """What the public functions return for a run_lattice(confidence="lines") result -> seconds, segments, scores.  scores[b] holds
    "occupancy", "onset_prob", "offset_prob" [L] (about the reported, FIRST visit; 0 for a character never sung), "path_log_posterior",
    "visits" [L] (the expected number of visits: it can exceed 1, and is constant along a line), "visit_occupancy" (one number per entry
    of segments[b]: the mean posterior of the reported state over that visit's frames), "line_visits" [M] (visits at each line's first
    character: the expected number of times the line is sung -- a count, not a probability) and "line_out_of_order" [M] (how many of
    them are expected to begin out of print order: by a jump or a free start; visits - in_order there, taken in float64)."""
    seconds = _seconds_from_frames(r.onset, r.offset, r.status, label_lists, hop_size_second, skipped_as_none=True)
    scores = _scores_from_posteriors(r.occupancy, r.onset_prob, r.offset_prob, r.log_z, r.score, label_lists)
    rows, pp = r.path.cpu().numpy(), r.path_prob.cpu().numpy()
    vis, ino, flags = r.visits.cpu().numpy().astype(np.float64), r.in_order.cpu().numpy().astype(np.float64), line_start.cpu().numpy()
    segments = []
    for b, T in enumerate(frame_counts):
        visits = _visits_of_row(rows[b, : int(T)])
        segments.append([(n, float(t) * hop_size_second, float(u) * hop_size_second) for n, t, u in visits])
        d, L = scores[b], len(label_lists[b])
        starts = [n for n in range(L) if flags[b, n] != 0]
        d["visits"] = [float(v) for v in vis[b, :L]]
        d["visit_occupancy"] = [float(pp[b, t:u].astype(np.float64).mean()) for _, t, u in visits]
        d["line_visits"] = [float(vis[b, a]) for a in starts]
        d["line_out_of_order"] = [float(vis[b, a] - ino[b, a]) for a in starts]
    return seconds, segments, scores


def _device_of(prediction) -> torch.device:
    _lib.require_gpu()
    if torch.is_tensor(prediction) and prediction.is_cuda:
        return prediction.device
    return torch.device(f"cuda:{torch.cuda.current_device()}")


def _repeat_rows(who: str, repeat_spans, return_segments: bool, label_lists, scored: bool):
    """The repeat_from rows a public function hands to run_lattice: _repeat_from_of_spans' where a span is given; all -1 where only the
    segments are asked for (the same result, with its path); None otherwise.  ValueError with any kind of confidence."""
    rows = _repeat_from_of_spans(repeat_spans, label_lists)
    if (rows is not None or return_segments) and scored:
        raise ValueError(f"{who}: repeat_spans / return_segments do not go with a confidence (no posteriors on the lattice with "
                         "repeatable spans)")
    if rows is None and return_segments:
        rows = torch.full((len(label_lists), max(1, max((len(l) for l in label_lists), default=1))), -1, dtype=torch.int32)
    return rows


def align_labels(who: str, emissions_of, lab, n_lab, label_lists, frame_counts, n_frames_max: int, nf, hop_size_second, confidence,
                 boundary_window, skip_from, windows, skip_penalty, optional_spans, repeat_spans, repeat_penalty, return_segments,
                 alternatives, return_readings, rd: Optional[Readings] = None, raw: bool = False, line_start=None, line_jump_penalty=0.0,
                 off: Optional[OffSheet] = None, return_off_sheet: bool = False, min_frames=None, pron: Optional[Pronunciation] = None):
    """What perform_viterbi* and AlignModel.align (`who`: "perform_viterbi" / "align") do once the labels (lab / n_lab on the device,
    label_lists), the spans and windows (host rows, or None) and the kind of confidence are known: the repeat_from rows
    (_repeat_from_of_spans for "repeat" / "song", whose label limit is refused here; _repeat_rows otherwise), the readings (rd: the
    caller's _readings_of result where it has one), the emissions, run_lattice, the reading scores, and the public return value --
    _formatted's or _formatted_repeat's, then the segments, then the readings; a bare result with readings becomes a tuple.
    emissions_of(labels, n_labels, needed=True) -> (dp, em): the compact emissions of the device label rows given (em; it may be None
    where `needed` is False and dp is not) and the plain lattice's (onset, offset, score, status) on them where the provider's kernel
    has them anyway (the fused head), else None.  With alternatives it is asked once, for the expanded rows; otherwise once for lab,
    with needed = "another lattice or a sweep reads the emissions" -- a dp without emissions is the result, and nothing else is launched.
    nf: the device frame counts of a ragged batch, or None: every clip has n_frames_max frames (filled here, and only if needed).
    raw: -> (the LatticeResult, ops.reading_scores' pair or ()) in place of the formatted value.
    pron (the caller's _pronunciation_of result, or None: the call as it was): the pronunciation scores.  emissions_of is asked ONCE for
    the widened rows (_widened_labels: the sheet's or the expanded rows, then the candidate classes); whatever DP result it brings is
    dropped, as the readings route drops it, and the lattice reads the leading columns of the widened matrix through its row stride.
    ops.segment_class_scores then runs on the trailing column window and the DP's onset / offset, with the sheet's class -- with
    alternatives the reading ops.reading_scores picked -- as the own class.  The return gains `pronunciation` as its last element
    (raw: ops.segment_class_scores' five tensors behind the reading pair).
    off (the caller's _off_sheet_of result, or None: the call as it was): off-sheet slots.  Every argument above is then the EXPANDED
    sheet's (off.label_lists and the remapped keywords).  emissions_of is asked for the expanded rows with needed=True and its DP
    result is dropped; with alternatives the fold comes first; then ops.offsheet_columns writes the slots' columns of the matrix the
    lattice reads, and run_lattice and everything behind it run unchanged on L' labels, the slots carrying OFF_SHEET_ID.  On the way out
    the slot entries leave every per-character output, segments go back to the caller's numbering and the dicts gain "off_sheet_prob"
    where they hold sung_prob / visits.  return_off_sheet: the return gains, as its last element, per clip the time-ordered list of
    {"position": n, "onset": s, "offset": s, "frames": k} of every slot visit (with pron also "top"); without slots empty lists.
    line_start (the caller's _line_start_of rows, or None: the call as it was) / line_jump_penalty: the lattice with free line order.  The
    caller has refused every keyword that does not go with it; the emissions are asked for, run_lattice takes the rows, and the result
    (a RepeatLatticeResult: first visits, the path for return_segments) goes through everything behind it unchanged.  confidence="lines"
    (only with a line_start: ValueError before the emissions are asked for) adds that lattice's sweep: -> (seconds, scores), or (seconds,
    segments, scores) with return_segments, the dicts _formatted_lines'; readings and pronunciation follow as ever.
    min_frames (the caller's _min_frames_of rows, or None: the call as it was): a floor, in frames, under every character's duration.  The
    caller has refused every keyword that does not go with it (ValueError here too, before the emissions are asked for); the emissions
    are asked for with needed=True, the provider's own plain DP result is dropped as the off-sheet route drops it, and
    run_min_duration_lattice takes the rows -- with alternatives the floors belong to the positions and the lattice reads the set ids.
    Its result (a RepeatLatticeResult: the path for return_segments) goes through everything behind it unchanged."""
    if min_frames is not None and (confidence is not None or skip_from is not None or windows is not None or line_start is not None
                                   or off is not None or _repeat_from_of_spans(repeat_spans, label_lists) is not None):
        raise ValueError(f"{who}: min_duration goes with the plain lattice alone (no spans, anchors, line order, off-sheet slots or "
                         "confidence)")
    if confidence == LINES_CONFIDENCE and line_start is None:
        raise ValueError(f"{who}: the line confidence is the posteriors of the lattice with free line order: it needs line_starts")
    repeat_kind = confidence in ("repeat", "song")
    if line_start is not None or min_frames is not None:
        repeat_from = None
    elif repeat_kind:
        repeat_from = _repeat_from_of_spans(repeat_spans, label_lists)
        if lab.shape[1] > POSTERIOR_MAX_LABELS and confidence == "repeat":
            raise NotImplementedError(f"{who}_repeat_scored: {lab.shape[1]} labels exceed the {POSTERIOR_MAX_LABELS}-label limit of "
                                      "the posteriors on the lattice with repeatable spans")
    else:
        repeat_from = _repeat_rows(who, repeat_spans, return_segments, label_lists, confidence is not None)
    # pronunciation alternatives: the head or the prep runs on the expanded labels and its matrix is folded in front of the lattice, which
    # sees the set-equality ids in the labels' place; None / all-empty takes the call as it was
    if rd is None:
        rd = _readings_of(alternatives, label_lists, keep_empty=return_readings)
    if off is not None and rd is not None:
        rd = rd._replace(lattice_ids=off.ids_with_slots(rd.lattice_ids))
    route, dp, em, em_c = None, None, None, None
    if pron is not None:
        classes, plain_emissions_of = torch.tensor(pron.classes, dtype=torch.int32).to(lab.device), emissions_of

        def emissions_of(lab_x, n_x, needed=True):
            nonlocal em_c
            em_w = plain_emissions_of(*_widened_labels(lab_x, n_x, classes), True)[1]
            em_c = em_w[:, :, 1 + lab_x.shape[1]:]
            return None, em_w[:, :, : 1 + lab_x.shape[1]]
    if rd is None:
        dp, em = emissions_of(lab, n_lab, confidence is not None or skip_from is not None or windows is not None or repeat_from is not None
                              or off is not None or line_start is not None or min_frames is not None)
        if off is not None or min_frames is not None:   # the provider's own DP ran without the slots' columns, or without the floors
            dp = None
    if rd is None and em is None:
        r = _result(dp)
    else:
        if nf is None:
            nf = torch.full((len(label_lists),), n_frames_max, dtype=torch.int32, device=lab.device)
        if rd is not None:
            route = readings_route(rd, lambda lab_x, n_x: emissions_of(lab_x, n_x)[1], n_lab, nf, lab.device)
            em, lab = route.em, route.lattice_ids
        if off is not None:
            ops.offsheet_columns(em, off.slot_cols.to(lab.device), off.n_slots.to(lab.device), nf, off.penalty)
            if route is None:
                lab = off.lattice_ids.to(lab.device)
        if min_frames is not None:
            r = run_min_duration_lattice(em, lab, n_lab, nf, min_frames)
        else:
            r = run_lattice(em, lab, n_lab, nf, skip_from, windows, skip_penalty, confidence, boundary_window, dp, repeat_from,
                            repeat_penalty, line_start, line_jump_penalty)
    picked = route.scores(n_lab, r.onset, r.offset) if return_readings or (pron is not None and route is not None) else ()
    if pron is not None:
        own_col = _own_columns(pron, route, picked[0] if route is not None else None, lab.device)
        scored = ops.segment_class_scores(em_c, n_lab, r.onset, r.offset, own_col, pron.top_k)
        picked = picked if return_readings else ()
    if raw:
        return (r, picked) if pron is None else (r, picked + scored)
    keep = (lambda rows: rows) if off is None else (lambda rows: [_without_slots(off, b, row) for b, row in enumerate(rows)])
    if repeat_kind:
        seconds, segments, scores = _formatted_repeat(r, label_lists, frame_counts, hop_size_second, optional_spans, repeat_spans)
        if off is not None:
            scores, segments = _scores_without_slots(off, scores, segments), _segments_without_slots(off, segments)
        out = (keep(seconds), segments, scores) if return_segments else (keep(seconds), scores)
    elif confidence == LINES_CONFIDENCE:
        seconds, segments, scores = _formatted_lines(r, label_lists, frame_counts, hop_size_second, line_start)
        out = (seconds, segments, scores) if return_segments else (seconds, scores)
    else:
        out = _formatted(r, label_lists, hop_size_second, optional_spans)
        out = (keep(out[0]), _scores_without_slots(off, out[1]) if off is not None else out[1]) if isinstance(out, tuple) else keep(out)
        if return_segments:
            segments = _segments_from_path(r.path, frame_counts, hop_size_second)
            out = (out, _segments_without_slots(off, segments) if off is not None else segments)
    if return_readings:
        readings = keep(_readings_from_scores(*picked, rd))
        out = (*out, readings) if isinstance(out, tuple) else (out, readings)
    if pron is not None:
        pronunciation = keep(_pronunciation_from_scores(scored, own_col, pron, label_lists))
        out = (*out, pronunciation) if isinstance(out, tuple) else (out, pronunciation)
    if return_off_sheet:
        heard = [[] for _ in label_lists]
        if off is not None:
            visits = _off_sheet_visits(off, r, frame_counts)
            top = _off_sheet_top(off, visits, em_c, pron, lab.device) if pron is not None else None
            heard = [[{"position": n, "onset": float(t) * hop_size_second, "offset": float(u) * hop_size_second, "frames": u - t,
                       **({"top": top[b][i]} if top is not None else {})} for i, (n, t, u) in enumerate(vis)] for b, vis in enumerate(visits)]
        out = (*out, heard) if isinstance(out, tuple) else (out, heard)
    return out


def _perform(prediction, labels, hop_size_second, variant, boundary_window=None, n_frames=None, optional_spans=None, skip_penalty=0.0,
             char_windows=None, onset_anchors=None, confidence=None, repeat_spans=None, repeat_penalty=0.0, return_segments=False,
             alternatives=None, return_readings=False, min_duration=None, line_starts=None, line_jump_penalty=0.0, off_sheet=None,
             off_sheet_penalty=DEFAULT_OFF_SHEET_PENALTY, return_off_sheet=False,
             return_pronunciation=False, pronunciation_classes=None, pronunciation_top_k=5):
    """confidence: the kind the public function stands for (run_lattice's); "plain" becomes "span" where a span is given (an off-sheet
    slot is one)."""
    if return_readings and alternatives is None:
        raise ValueError("return_readings goes with alternatives (without them every character has the one reading of its label)")
    rd = pron = off = None
    # minimum duration: every refusal and the rows, before anything is on a device
    _min_duration_alone("perform_viterbi", min_duration, optional_spans=optional_spans, repeat_spans=repeat_spans, onset_anchors=onset_anchors,
                        char_windows=char_windows, line_starts=line_starts, off_sheet=off_sheet, confidence=confidence)
    min_frames = _min_frames_of("perform_viterbi", min_duration, _label_lists(labels, len(labels)), hop_size_second)
    # free line order: the rows and every refusal, before anything is on a device
    _line_starts_alone("perform_viterbi", line_starts, optional_spans=optional_spans, repeat_spans=repeat_spans, onset_anchors=onset_anchors,
                       char_windows=char_windows, off_sheet=off_sheet, confidence=None if confidence == LINES_CONFIDENCE else confidence)
    if confidence == LINES_CONFIDENCE and line_starts is None:
        raise ValueError("perform_viterbi_line_confidence: line_starts is required (the posteriors of the lattice with free line order)")
    line_start = _line_start_of("perform_viterbi", line_starts, _label_lists(labels, len(labels)))
    if line_start is not None and not float(line_jump_penalty) >= 0.0:
        raise ValueError("perform_viterbi: line_jump_penalty must be >= 0")
    if off_sheet is not None:                # off-sheet slots: from here on the sheet is the expanded one, the keywords are remapped
        off = _off_sheet_of("perform_viterbi", off_sheet, off_sheet_penalty, _label_lists(labels, len(labels)), optional_spans, repeat_spans,
                            char_windows, onset_anchors, alternatives, narrow=confidence in ("plain", "span", "anchored", "repeat"))
    if off is not None:
        labels, optional_spans, repeat_spans = off.label_lists, off.optional_spans, off.repeat_spans
        char_windows, onset_anchors, alternatives = off.char_windows, off.onset_anchors, off.alternatives
    if return_pronunciation:                 # the keyword checks, before anything is on a device
        lists = _label_lists(labels, len(labels))
        rd = _readings_of(alternatives, lists, keep_empty=return_readings)
        pron = _pronunciation_of("perform_viterbi", True, pronunciation_classes, pronunciation_top_k, lists, rd,
                                 None if off is None else off.slot_sets())
    dev = _device_of(prediction)
    pred = torch.as_tensor(prediction).to(device=dev, dtype=torch.float32)
    if pred.dim() != 3:
        raise ValueError("prediction must be [B, T, V]")
    if pred.stride(2) != 1:
        pred = pred.contiguous()
    B, T, V = pred.shape
    lab, n_lab, lists = _labels_to_device(labels, B, dev)
    counts, nf = [T] * B, None
    if n_frames is not None:                 # (addition) utterance b owns the first n_frames[b] rows of a zero-padded [B, Tmax, V] prediction
        counts = [int(v) for v in (n_frames.tolist() if torch.is_tensor(n_frames) else n_frames)]
        if len(counts) != B or any(v < 0 or v > T for v in counts):
            raise ValueError(f"n_frames: {B} frame counts in 0..{T} expected")
        nf = torch.tensor(counts, dtype=torch.int32).to(dev)
    # (additions) optional spans and per-state frame windows; None / all-empty keywords take the reference's lattice unchanged
    skip_from = _skip_from_of_spans(optional_spans, lists)
    windows = _windows_of(char_windows, onset_anchors, lists, counts, hop_size_second)
    if windows is not None and confidence == "plain":
        raise ValueError("char_windows / onset_anchors: the _scored functions have no posteriors on the windowed lattice "
                         "(perform_viterbi(_ctc)_anchored_scored give them)")
    if confidence == "plain" and skip_from is not None:
        confidence = "span"
    return align_labels("perform_viterbi", lambda lab_x, n_x, needed=True: (None, ops.emissions_from_logits(pred, lab_x, n_x, variant)), lab,
                        n_lab, lists, counts, T, nf, hop_size_second, confidence, boundary_window, skip_from, windows, skip_penalty,
                        optional_spans, repeat_spans, repeat_penalty, return_segments, alternatives, return_readings, rd, pron=pron,
                        off=off, return_off_sheet=return_off_sheet, line_start=line_start, line_jump_penalty=float(line_jump_penalty),
                        min_frames=min_frames)


def perform_viterbi(prediction, labels, hop_size_second=0.02, n_frames=None, optional_spans=None, skip_penalty=0.0,
                    char_windows=None, onset_anchors=None, repeat_spans=None, repeat_penalty=0.0, return_segments=False, alternatives=None, return_readings=False,
                    min_duration=None, line_starts=None, line_jump_penalty=0.0,
                    off_sheet=None, off_sheet_penalty=DEFAULT_OFF_SHEET_PENALTY, return_off_sheet=False,
                    return_pronunciation=False, pronunciation_classes=None, pronunciation_top_k=5):
    """n_frames (addition; the reference has none): per-utterance frame counts for a zero-padded [B, Tmax, V] prediction -- utterance b is
    aligned over its first n_frames[b] rows, as if it had been handed over alone.
    optional_spans (addition): optional_spans[b] = list of (a, n) pairs, labels a .. n-1 of utterance b may be left out by the path
    (la_viterbi_spans_batch; skip_penalty >= 0 per taken jump); skipped characters come back as None in place of [onset, offset].
    None or all-empty: today's DP.  ValueError for a < 0, a >= n, n > L or two spans with one end.
    char_windows / onset_anchors (addition): per utterance a list in windows_from_anchors' form (seconds, in the utterance's own frames):
    the DP runs on the lattice with per-state frame windows (la_viterbi_windows_batch), with or without optional_spans.  None or
    all-empty: the call as it was.  An utterance without a path inside its windows raises like one too short for its labels.
    Up to 4095 labels with any of these keywords (beyond 511 the DP is la_viterbi_lattice_batch); the _scored functions at most 511,
    except perform_viterbi(_ctc)_sheet_scored, which take whole songs (up to 4095).
    repeat_spans (addition): repeat_spans[b] = list of (a, e) pairs -- having sung label e-1 of utterance b the path may return to label
    a (a chorus printed once and sung twice; la_viterbi_repeats_batch, repeat_penalty >= 0 per return, the only control of how often).
    The result keeps its shape: the FIRST visit per character, None for a character never visited.  ValueError for a < 0, a >= e, e > L
    or two spans with one start.  With optional_spans, char_windows / onset_anchors and n_frames, up to 4095 labels; the older _scored
    functions and anchored_alignment_loss raise ValueError with it (perform_viterbi(_ctc)_repeat_scored: its confidence, up to 511
    labels; perform_viterbi(_ctc)_song_scored: up to 4095).  None or all-empty: the call as it was.
    return_segments (addition): -> (predicted_onset_offset, segments), segments[b] = the time-ordered list of (char_index, onset_s,
    offset_s) of EVERY visit, with or without repeat_spans.
    alternatives (addition; here and in perform_viterbi_ctc and every _scored function): alternatives[b] = [(n, [class, ...]), ...] -- label n
    of utterance b may also be sung as one of these classes (a character with several readings; at most 8 readings per position, the
    sheet's own included, at most 4095 expanded columns per utterance: _readings_of).  The position's lattice state is scored on the
    merged class, log sum exp over its readings per frame (la_emissions_merge_readings on the prep's emissions for the expanded labels);
    two neighbouring positions count as the same label exactly when their reading sets are equal.  With every other keyword; the
    confidences are then posteriors of the merged class.  None or all-empty: the call as it was.
    return_readings (with alternatives; ValueError without): the return gains `readings` as its last element (a bare result becomes
    (result, readings)): readings[b][n] = (class id sung, [score per reading, the sheet's own class first]) -- the score of a reading is
    the sum of its emissions over the segment the DP chose (the reported visit), the class the smallest index with the largest score
    (la_reading_scores) -- or None for a skipped character.
    return_pronunciation / pronunciation_classes / pronunciation_top_k (addition; here and in perform_viterbi_ctc): was the sheet's
    character the one that was sung?  pronunciation_classes (required: ValueError without) is an int N -- classes 1 .. N -- or a sequence of
    class ids; the sheet's own classes are unioned in, the list sorted and unique; with the label columns at most 4095 columns
    (NotImplementedError before anything is launched).  The prep runs once on the sheet's rows followed by the candidate classes, the
    lattice on the leading columns of that matrix, and la_segment_class_scores sums every candidate over the segment the DP chose (the
    reported, first visit).  The return gains `pronunciation` as its last element, after `readings`: pronunciation[b][n] = None for a
    skipped character, else {"class": the own class id (with alternatives the reading picked), "frames": n, "log_prob": own_score / n,
    "rank": the number of candidates that beat the own class (0 = it is the best), "gop": (own_score - best score) / n <= 0, 0.0 at
    rank 0, "top": [(class id, score / n), ...] the pronunciation_top_k (1 .. 16) best}.  With every other keyword; off: the call as it
    was.  No threshold on gop is calibrated: none has been measured on real singing.
    line_starts / line_jump_penalty (addition; here and in perform_viterbi_ctc): an UNMARKED sheet whose lines may be sung in any order, any
    number of times or not at all.  line_starts[b] = [0, 7, 15, ...], the label indices at which a line of utterance b begins -- the
    line breaks and nothing else (la_viterbi_lines_batch): after the last character of any line the path may go on to the first
    character of any line, it may begin at any line's start and stop at any line's end, each such jump charged line_jump_penalty >= 0
    (the default 0.0 follows skip_penalty / repeat_penalty and HAS NOT BEEN TUNED on real singing).  The result keeps its shape: the
    FIRST visit per character, None for a character never sung; return_segments gives every visit in time order.  With n_frames,
    alternatives / return_readings and return_pronunciation (both read the first visit), up to 4095 labels (NotImplementedError).
    ValueError for a row that does not begin with 0, is not strictly ascending or holds an index >= L_b, and together with
    optional_spans, repeat_spans, onset_anchors, char_windows or off_sheet; the _scored functions and the training entries do not have
    the keyword.  None: the call as it was.
    off_sheet / off_sheet_penalty / return_off_sheet (addition; here, in perform_viterbi_ctc and every _scored function): singing that is
    in the audio but not on the sheet (ad-libs, backing vocals, an omitted verse, a partial sheet).  off_sheet[b] = [n, ...] puts a SLOT
    before label n of utterance b (0 <= n <= L_b; L_b = after the last label): a label position of its own whose emission is
    log P(frame is not silence) - off_sheet_penalty (la_emissions_offsheet_columns on column 0 of the prep's matrix), skippable by a
    one-label optional span.  The slot beats the sheet's character on a frame when that character holds less than exp(-penalty) of the
    voiced probability; the default ln 100 (a 1 % share, nats per frame) HAS NOT BEEN TUNED on real singing.  The other keywords keep the
    caller's numbering (a slot strictly inside an optional or repeat span belongs to it) and every per-character output keeps its
    shape.  return_off_sheet: the return gains, as its last element, off_sheet[b] = the time-ordered list of {"position": n, "onset": s,
    "offset": s, "frames": k}, one per slot visit (unused slots are absent; with return_pronunciation also "top": [(class id, score per
    frame), ...], what was heard there).  The _scored functions that report sung_prob / visits add "off_sheet_prob": {n: value} for
    every slot.  Two properties of the lattice: with a slot before the first label the first character cannot start at frame 0 (after
    the last: the last character cannot end on the last frame); and an unused slot is charged skip_penalty like every skipped span, so
    keep off_sheet_penalty above skip_penalty.  ValueError for a wrong list count, a bad or repeated n, a slot on an utterance without
    labels or a negative / NaN penalty; NotImplementedError when L_b plus its slots exceed 4095 (511 for the confidences that stop
    there).  None or all-empty: the call as it was.
    min_duration (addition; here and in perform_viterbi_ctc): a floor under every character's duration -- a sung syllable is never one
    20 ms frame long, and the plain lattice lets it be.  One number of seconds for every character, or per utterance a row of
    per-character seconds (a None row: no floor there); a floor is ceil(seconds / hop_size_second - 1e-9) frames, at least 1 and at
    most 8 (160 ms at the model's hop).  The DP is la_viterbi_min_duration_batch on the plain lattice: every reported character lasts
    at least its floor, the last one included, and an utterance too short for its floors raises like one too short for its labels.
    With n_frames, alternatives / return_readings (floors belong to positions), return_pronunciation and return_segments, up to 4095
    labels.  ValueError for a negative or non-finite value, a wrong row count or length or a floor above 8 frames, and together with
    optional_spans, repeat_spans, onset_anchors, char_windows, line_starts or off_sheet; the _scored functions and the training
    entries do not have the keyword (no posteriors exist on this lattice yet).  None, or every floor at most one frame: the call as
    it was, launch for launch.  No floor HAS BEEN TUNED on real singing, so there is no default."""
    return _perform(prediction, labels, hop_size_second, LA_VARIANT_PLAIN, n_frames=n_frames, optional_spans=optional_spans,
                    skip_penalty=skip_penalty, char_windows=char_windows, onset_anchors=onset_anchors, repeat_spans=repeat_spans,
                    repeat_penalty=repeat_penalty, return_segments=return_segments, alternatives=alternatives, return_readings=return_readings,
                    min_duration=min_duration, line_starts=line_starts, line_jump_penalty=line_jump_penalty,
                    return_pronunciation=return_pronunciation, pronunciation_classes=pronunciation_classes,
                    pronunciation_top_k=pronunciation_top_k,
                    off_sheet=off_sheet, off_sheet_penalty=off_sheet_penalty, return_off_sheet=return_off_sheet)


def perform_viterbi_ctc(prediction, labels, hop_size_second=0.02, n_frames=None, optional_spans=None, skip_penalty=0.0,
                        char_windows=None, onset_anchors=None, repeat_spans=None, repeat_penalty=0.0, return_segments=False, alternatives=None, return_readings=False,
                        min_duration=None, line_starts=None, line_jump_penalty=0.0,
                        off_sheet=None, off_sheet_penalty=DEFAULT_OFF_SHEET_PENALTY, return_off_sheet=False,
                        return_pronunciation=False, pronunciation_classes=None, pronunciation_top_k=5):
    return _perform(prediction, labels, hop_size_second, LA_VARIANT_CTC, n_frames=n_frames, optional_spans=optional_spans,
                    skip_penalty=skip_penalty, char_windows=char_windows, onset_anchors=onset_anchors, repeat_spans=repeat_spans,
                    repeat_penalty=repeat_penalty, return_segments=return_segments, alternatives=alternatives, return_readings=return_readings,
                    min_duration=min_duration, line_starts=line_starts, line_jump_penalty=line_jump_penalty,
                    return_pronunciation=return_pronunciation, pronunciation_classes=pronunciation_classes,
                    pronunciation_top_k=pronunciation_top_k,
                    off_sheet=off_sheet, off_sheet_penalty=off_sheet_penalty, return_off_sheet=return_off_sheet)


def perform_viterbi_scored(prediction, labels, hop_size_second=0.02, boundary_window=2, n_frames=None, optional_spans=None, skip_penalty=0.0,
                           char_windows=None, onset_anchors=None, repeat_spans=None, alternatives=None, return_readings=False,
                           off_sheet=None, off_sheet_penalty=DEFAULT_OFF_SHEET_PENALTY, return_off_sheet=False):
    """perform_viterbi plus per-character confidence (addition; the reference has none): -> (predicted_onset_offset, scores),
    scores[b] = {"occupancy": [L], "onset_prob": [L], "offset_prob": [L], "path_log_posterior": float} from the forward-backward
    sweep of the same lattice (include/lyricalign.h la_alignment_posteriors).  Same exceptions as perform_viterbi.
    optional_spans / skip_penalty as perform_viterbi: skipped characters are None (their three scores 0), and each dict additionally holds
    "sung_prob": [L] (probability that the character is on the path at all) and "span_skip_prob": one value per span, in the order given
    (probability that the span was left out) -- la_alignment_posteriors_spans.  Without a span the dicts are as before, without these keys.
    char_windows / onset_anchors: ValueError unless None or all-empty (perform_viterbi_anchored_scored is the function for them).
    repeat_spans: ValueError unless None or all-empty, here and in the anchored / sheet _scored functions
    (perform_viterbi(_ctc)_repeat_scored give the posteriors of that lattice)."""
    return _perform(prediction, labels, hop_size_second, LA_VARIANT_PLAIN, int(boundary_window), n_frames=n_frames,
                    optional_spans=optional_spans, skip_penalty=skip_penalty, char_windows=char_windows, onset_anchors=onset_anchors,
                    confidence="plain", repeat_spans=repeat_spans, alternatives=alternatives, return_readings=return_readings,
                    off_sheet=off_sheet, off_sheet_penalty=off_sheet_penalty, return_off_sheet=return_off_sheet)


def perform_viterbi_ctc_scored(prediction, labels, hop_size_second=0.02, boundary_window=2, n_frames=None, optional_spans=None,
                               skip_penalty=0.0, char_windows=None, onset_anchors=None, repeat_spans=None, alternatives=None, return_readings=False,
                               off_sheet=None, off_sheet_penalty=DEFAULT_OFF_SHEET_PENALTY, return_off_sheet=False):
    """perform_viterbi_ctc plus per-character confidence: see perform_viterbi_scored."""
    return _perform(prediction, labels, hop_size_second, LA_VARIANT_CTC, int(boundary_window), n_frames=n_frames,
                    optional_spans=optional_spans, skip_penalty=skip_penalty, char_windows=char_windows, onset_anchors=onset_anchors,
                    confidence="plain", repeat_spans=repeat_spans, alternatives=alternatives, return_readings=return_readings,
                    off_sheet=off_sheet, off_sheet_penalty=off_sheet_penalty, return_off_sheet=return_off_sheet)


def perform_viterbi_anchored_scored(prediction, labels, hop_size_second=0.02, boundary_window=2, n_frames=None, optional_spans=None,
                                    skip_penalty=0.0, char_windows=None, onset_anchors=None, repeat_spans=None, alternatives=None, return_readings=False,
                                    off_sheet=None, off_sheet_penalty=DEFAULT_OFF_SHEET_PENALTY, return_off_sheet=False):
    """perform_viterbi with char_windows / onset_anchors plus the confidence GIVEN them (addition): -> (predicted_onset_offset, scores).
    The DP and the forward-backward sweep run on the lattice with per-state frame windows (la_viterbi_windows_batch,
    la_alignment_posteriors_windows), with or without optional_spans.  scores[b] holds perform_viterbi_scored's keys with optional_spans
    ("occupancy", "onset_prob", "offset_prob", "path_log_posterior", "sung_prob", "span_skip_prob"; without a span sung_prob is 1 and
    span_skip_prob empty), every one a posterior given the windows, and "window_log_prob" = log_z(windowed) - log_z(same lattice, no
    windows) <= 0: the log-probability the unanchored model gives to "the path lies inside the windows" -- near 0 when the anchors agree
    with the audio, strongly negative when one of them fights it.  None or all-empty windows: the unanchored numbers and
    window_log_prob 0.0.  An utterance without a path inside its windows raises as in perform_viterbi."""
    return _perform(prediction, labels, hop_size_second, LA_VARIANT_PLAIN, int(boundary_window), n_frames=n_frames,
                    optional_spans=optional_spans, skip_penalty=skip_penalty, char_windows=char_windows, onset_anchors=onset_anchors,
                    confidence="anchored",
                    repeat_spans=repeat_spans, alternatives=alternatives, return_readings=return_readings,
                    off_sheet=off_sheet, off_sheet_penalty=off_sheet_penalty, return_off_sheet=return_off_sheet)


def perform_viterbi_ctc_anchored_scored(prediction, labels, hop_size_second=0.02, boundary_window=2, n_frames=None, optional_spans=None,
                                        skip_penalty=0.0, char_windows=None, onset_anchors=None, repeat_spans=None, alternatives=None, return_readings=False,
                                        off_sheet=None, off_sheet_penalty=DEFAULT_OFF_SHEET_PENALTY, return_off_sheet=False):
    """perform_viterbi_ctc plus the confidence given the windows: see perform_viterbi_anchored_scored."""
    return _perform(prediction, labels, hop_size_second, LA_VARIANT_CTC, int(boundary_window), n_frames=n_frames,
                    optional_spans=optional_spans, skip_penalty=skip_penalty, char_windows=char_windows, onset_anchors=onset_anchors,
                    confidence="anchored",
                    repeat_spans=repeat_spans, alternatives=alternatives, return_readings=return_readings,
                    off_sheet=off_sheet, off_sheet_penalty=off_sheet_penalty, return_off_sheet=return_off_sheet)


def perform_viterbi_sheet_scored(prediction, labels, hop_size_second=0.02, boundary_window=2, n_frames=None, optional_spans=None,
                                 skip_penalty=0.0, char_windows=None, onset_anchors=None, repeat_spans=None, alternatives=None, return_readings=False,
                                 off_sheet=None, off_sheet_penalty=DEFAULT_OFF_SHEET_PENALTY, return_off_sheet=False):
    """Whole-song timing with its confidences (addition): perform_viterbi_anchored_scored's (predicted_onset_offset, scores) for up to 4095
    labels, with or without optional_spans and char_windows / onset_anchors (la_viterbi_lattice_batch's routing for the DP,
    la_alignment_posteriors_lattice for the posteriors).  window_log_prob is 0.0 without windows.  Up to 511 labels the numbers are
    perform_viterbi_anchored_scored's exactly.  The sweep's workspace holds every alpha row: T * 1024 R * 8 bytes per utterance beyond
    511 labels (R = 2 / 4 / 8 for up to 1023 / 2047 / 4095 labels)."""
    return _perform(prediction, labels, hop_size_second, LA_VARIANT_PLAIN, int(boundary_window), n_frames=n_frames,
                    optional_spans=optional_spans, skip_penalty=skip_penalty, char_windows=char_windows, onset_anchors=onset_anchors,
                    confidence="sheet",
                    repeat_spans=repeat_spans, alternatives=alternatives, return_readings=return_readings,
                    off_sheet=off_sheet, off_sheet_penalty=off_sheet_penalty, return_off_sheet=return_off_sheet)


def perform_viterbi_ctc_sheet_scored(prediction, labels, hop_size_second=0.02, boundary_window=2, n_frames=None, optional_spans=None,
                                     skip_penalty=0.0, char_windows=None, onset_anchors=None, repeat_spans=None, alternatives=None, return_readings=False,
                                     off_sheet=None, off_sheet_penalty=DEFAULT_OFF_SHEET_PENALTY, return_off_sheet=False):
    """perform_viterbi_ctc plus the whole-song confidences: see perform_viterbi_sheet_scored."""
    return _perform(prediction, labels, hop_size_second, LA_VARIANT_CTC, int(boundary_window), n_frames=n_frames,
                    optional_spans=optional_spans, skip_penalty=skip_penalty, char_windows=char_windows, onset_anchors=onset_anchors,
                    confidence="sheet",
                    repeat_spans=repeat_spans, alternatives=alternatives, return_readings=return_readings,
                    off_sheet=off_sheet, off_sheet_penalty=off_sheet_penalty, return_off_sheet=return_off_sheet)


def perform_viterbi_repeat_scored(prediction, labels, hop_size_second=0.02, boundary_window=2, n_frames=None, optional_spans=None,
                                  skip_penalty=0.0, char_windows=None, onset_anchors=None, repeat_spans=None, repeat_penalty=0.0,
                                  return_segments=False, alternatives=None, return_readings=False,
                                  off_sheet=None, off_sheet_penalty=DEFAULT_OFF_SHEET_PENALTY, return_off_sheet=False):
    """perform_viterbi with repeat_spans plus the confidence of that lattice (addition): -> (predicted_onset_offset, scores), or
    (predicted_onset_offset, segments, scores) with return_segments.  The DP is la_viterbi_repeats_batch, the sweep
    la_alignment_posteriors_repeats, with or without optional_spans, char_windows / onset_anchors and n_frames; up to 511 labels
    (NotImplementedError before anything is launched; perform_viterbi_song_scored takes whole songs).  A path may visit a character more than once on this lattice, so some numbers are
    EXPECTED COUNTS, can exceed 1 and are not clamped.  scores[b] holds
      "occupancy", "onset_prob", "offset_prob" [L]: about the reported (first) visit; onset_prob / offset_prob count the visits that begin /
          end within boundary_window frames of the reported boundary (probabilities unless two visits can begin that close together);
      "path_log_posterior": final_score - log_z <= 0;
      "visits" [L]: the expected number of times the character is sung (sung_prob where no repeat span exists);
      "repeat_count": {(a, e): the expected number of returns of that span} for the spans of repeat_spans[b];
      "span_skip_prob": one value per span of optional_spans[b] (an expected count where a repeat span covers the optional span);
      "visit_occupancy": one number per entry of segments[b], the mean posterior of the reported state over that visit's frames -- the
          occupancy of every visit, not only the first;
      "window_log_prob" (only where char_windows / onset_anchors are given): log_z(windowed) - log_z(same lattice, no windows) <= 0, from
          a second sweep without them.
    With no repeat span anywhere the numbers it shares with perform_viterbi_sheet_scored are that function's exactly."""
    return _perform(prediction, labels, hop_size_second, LA_VARIANT_PLAIN, int(boundary_window), n_frames=n_frames,
                    optional_spans=optional_spans, skip_penalty=skip_penalty, char_windows=char_windows, onset_anchors=onset_anchors,
                    repeat_spans=repeat_spans, repeat_penalty=repeat_penalty, return_segments=return_segments, confidence="repeat", alternatives=alternatives, return_readings=return_readings,
                    off_sheet=off_sheet, off_sheet_penalty=off_sheet_penalty, return_off_sheet=return_off_sheet)


def perform_viterbi_ctc_repeat_scored(prediction, labels, hop_size_second=0.02, boundary_window=2, n_frames=None, optional_spans=None,
                                      skip_penalty=0.0, char_windows=None, onset_anchors=None, repeat_spans=None, repeat_penalty=0.0,
                                      return_segments=False, alternatives=None, return_readings=False,
                                      off_sheet=None, off_sheet_penalty=DEFAULT_OFF_SHEET_PENALTY, return_off_sheet=False):
    """perform_viterbi_ctc plus the confidence of the lattice with repeatable spans: see perform_viterbi_repeat_scored."""
    return _perform(prediction, labels, hop_size_second, LA_VARIANT_CTC, int(boundary_window), n_frames=n_frames,
                    optional_spans=optional_spans, skip_penalty=skip_penalty, char_windows=char_windows, onset_anchors=onset_anchors,
                    repeat_spans=repeat_spans, repeat_penalty=repeat_penalty, return_segments=return_segments, confidence="repeat", alternatives=alternatives, return_readings=return_readings,
                    off_sheet=off_sheet, off_sheet_penalty=off_sheet_penalty, return_off_sheet=return_off_sheet)


def perform_viterbi_song_scored(prediction, labels, hop_size_second=0.02, boundary_window=2, n_frames=None, optional_spans=None,
                                skip_penalty=0.0, char_windows=None, onset_anchors=None, repeat_spans=None, repeat_penalty=0.0,
                                return_segments=False, alternatives=None, return_readings=False,
                                off_sheet=None, off_sheet_penalty=DEFAULT_OFF_SHEET_PENALTY, return_off_sheet=False):
    """Whole-song timing with repeated lines and its confidences (addition): perform_viterbi_repeat_scored's arguments and return values
    for up to 4095 labels (la_viterbi_repeats_batch for the DP, la_alignment_posteriors_song for the posteriors).  Up to 511 labels
    the numbers are perform_viterbi_repeat_scored's exactly.  The sweep's workspace holds every alpha row: T * 1024 R * 8 bytes per
    utterance beyond 511 labels (R = 2 / 4 / 8 for up to 1023 / 2047 / 4095 labels)."""
    return _perform(prediction, labels, hop_size_second, LA_VARIANT_PLAIN, int(boundary_window), n_frames=n_frames,
                    optional_spans=optional_spans, skip_penalty=skip_penalty, char_windows=char_windows, onset_anchors=onset_anchors,
                    repeat_spans=repeat_spans, repeat_penalty=repeat_penalty, return_segments=return_segments, confidence="song", alternatives=alternatives, return_readings=return_readings,
                    off_sheet=off_sheet, off_sheet_penalty=off_sheet_penalty, return_off_sheet=return_off_sheet)


def perform_viterbi_ctc_song_scored(prediction, labels, hop_size_second=0.02, boundary_window=2, n_frames=None, optional_spans=None,
                                    skip_penalty=0.0, char_windows=None, onset_anchors=None, repeat_spans=None, repeat_penalty=0.0,
                                    return_segments=False, alternatives=None, return_readings=False,
                                    off_sheet=None, off_sheet_penalty=DEFAULT_OFF_SHEET_PENALTY, return_off_sheet=False):
    """perform_viterbi_ctc plus the whole-song confidences of the lattice with repeatable spans: see perform_viterbi_song_scored."""
    return _perform(prediction, labels, hop_size_second, LA_VARIANT_CTC, int(boundary_window), n_frames=n_frames,
                    optional_spans=optional_spans, skip_penalty=skip_penalty, char_windows=char_windows, onset_anchors=onset_anchors,
                    repeat_spans=repeat_spans, repeat_penalty=repeat_penalty, return_segments=return_segments, confidence="song", alternatives=alternatives, return_readings=return_readings,
                    off_sheet=off_sheet, off_sheet_penalty=off_sheet_penalty, return_off_sheet=return_off_sheet)


def perform_viterbi_line_confidence(prediction, labels, line_starts, line_jump_penalty=0.0, boundary_window=2, hop_size_second=0.02,
                                    n_frames=None, return_segments=False, alternatives=None, return_readings=False,
                                    return_pronunciation=False, pronunciation_classes=None, pronunciation_top_k=5):
    """perform_viterbi with line_starts plus the confidence of that lattice (addition): -> (predicted_onset_offset, scores), or
    (predicted_onset_offset, segments, scores) with return_segments.  The DP is la_viterbi_lines_batch, the sweep
    la_alignment_posteriors_lines on the same emissions, up to 4095 labels; line_starts is required (ValueError for None), and
    line_jump_penalty (default 0.0) has not been tuned on real singing.  A path may sing a line any number of times, so some numbers are
    EXPECTED COUNTS, can exceed 1 and are not clamped.  scores[b] holds
      "occupancy", "onset_prob", "offset_prob" [L]: about the reported (first) visit, 0 for a character never sung;
      "path_log_posterior": final_score - log_z <= 0, the log-probability of the reported order and timing together;
      "visits" [L]: the expected number of times the character is sung (constant along a line);
      "visit_occupancy": one number per entry of segments[b], the mean posterior of the reported state over that visit's frames;
      "line_visits" [M]: per line the expected number of times it is sung -- a count, not a probability;
      "line_out_of_order" [M]: per line how many of those are expected to begin out of print order (by a jump or a free start).
    With n_frames, alternatives / return_readings and return_pronunciation as perform_viterbi with line_starts.  The sweep's workspace
    holds every alpha row and every line start's jump term: T * 1.5 * (states per workgroup) * 8 bytes per utterance."""
    return _perform(prediction, labels, hop_size_second, LA_VARIANT_PLAIN, int(boundary_window), n_frames=n_frames, confidence=LINES_CONFIDENCE,
                    return_segments=return_segments, alternatives=alternatives, return_readings=return_readings, line_starts=line_starts,
                    line_jump_penalty=line_jump_penalty, return_pronunciation=return_pronunciation,
                    pronunciation_classes=pronunciation_classes, pronunciation_top_k=pronunciation_top_k)


def perform_viterbi_ctc_line_confidence(prediction, labels, line_starts, line_jump_penalty=0.0, boundary_window=2, hop_size_second=0.02,
                                        n_frames=None, return_segments=False, alternatives=None, return_readings=False,
                                        return_pronunciation=False, pronunciation_classes=None, pronunciation_top_k=5):
    """perform_viterbi_ctc plus the confidence of the lattice with free line order: see perform_viterbi_line_confidence."""
    return _perform(prediction, labels, hop_size_second, LA_VARIANT_CTC, int(boundary_window), n_frames=n_frames, confidence=LINES_CONFIDENCE,
                    return_segments=return_segments, alternatives=alternatives, return_readings=return_readings, line_starts=line_starts,
                    line_jump_penalty=line_jump_penalty, return_pronunciation=return_pronunciation,
                    pronunciation_classes=pronunciation_classes, pronunciation_top_k=pronunciation_top_k)


class _AnchoredAlignmentLoss(torch.autograd.Function):
    """finetune.anchored_alignment_loss under autograd: the loss kernels write d loss / d logits in the forward, backward hands it on
    (times the incoming scalar: the chain rule's factor, 1 for a plain loss.backward())."""

    @staticmethod
    def forward(ctx, align_logit, lab, lo, hi, nf, skip, skip_penalty, vocab_size):
        from ..finetune import anchored_alignment_loss as loss_kernels
        want = align_logit.requires_grad
        loss, nll, status, dlogits = loss_kernels(align_logit.detach().contiguous(), lab, lo, hi, nf, skip, skip_penalty,
                                                  vocab_size=vocab_size, scale=1.0, want_grad=want)
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(nll, status)
        return loss.view(()), nll, status

    @staticmethod
    def backward(ctx, grad_loss, _grad_nll, _grad_status):
        (dlogits,) = ctx.saved_tensors
        return (None if dlogits is None else dlogits * grad_loss, None, None, None, None, None, None, None)


def anchored_loss_inputs(labels, frame_counts: Sequence[int], onset_anchors=None, char_windows=None, optional_spans=None,
                         hop_size_second: float = 0.02):
    """What finetune.anchored_alignment_loss takes beside the logits, from the keywords of AlignModel.align (host only): labels [B, Lmax]
    (tensor / array / lists, -100 padding) -> (labels int64 [B, Lmax] with -100 padding, (win_lo, win_hi) int32 [B, 2 Lmax + 1] by
    _windows_of -- every window open when nothing is known about time --, skip_from int32 [B, Lmax + 1] by _skip_from_of_spans or None)."""
    B = len(frame_counts)
    lab_t = torch.as_tensor(labels)
    lists = _label_lists(lab_t.cpu() if torch.is_tensor(lab_t) else lab_t, B)
    Lmax = max(1, max((len(l) for l in lists), default=1))
    lab = torch.full((B, Lmax), -100, dtype=torch.int64)
    for b, l in enumerate(lists):
        if l:
            lab[b, : len(l)] = torch.tensor(l, dtype=torch.int64)
    skip = _skip_from_of_spans(optional_spans, lists)
    windows = _windows_of(char_windows, onset_anchors, lists, frame_counts, hop_size_second)
    if windows is None:                       # nothing known about time: every window is open
        windows = (torch.zeros((B, 2 * Lmax + 1), dtype=torch.int32),
                   torch.tensor([int(v) for v in frame_counts], dtype=torch.int32)[:, None].repeat(1, 2 * Lmax + 1))
    return lab, windows, skip


def anchored_alignment_loss(align_logit, labels, onset_anchors=None, char_windows=None, optional_spans=None, skip_penalty=0.0,
                            hop_size_second=0.02, n_frames=None, on_infeasible="raise", repeat_spans=None, alternatives=None,
                            return_pronunciation=False):
    """Training from line times (addition; the reference's losses need a label for every frame): -log of the total weight of the alignments
    that char_windows / onset_anchors (per utterance, in windows_from_anchors' form, seconds in the utterance's own frames) and
    optional_spans (as perform_viterbi) allow, per frame and averaged over the batch -- include/lyricalign.h la_anchored_alignment_loss.
    With every frame pinned to one state this is the frame CE + silence BCE of train_multitask.py:587-614 with hard targets; with looser
    windows it is that loss marginalised over the alignments.  No constraint at all is legal: every window is open.
    align_logit [B, T, V+1] float32 on the device (AlignModel.frame_manual_forward in .train(); column V = the silence logit: the CTC
    variant, the only one); labels [B, Lmax] class ids with -100 padding; n_frames as perform_viterbi.
    -> a device scalar with a grad_fn: `loss.backward(); optimizer.step()` works with it.
    on_infeasible: "raise" reads the per-clip status once (ONE host synchronisation per call) and raises ValueError naming the first clip
    without a path inside its windows (or without labels); "skip" does not read it: such a clip adds nothing to the loss (still divided by
    B) and gets a zero gradient.
    repeat_spans: ValueError unless None or all-empty (the loss does not know the lattice with repeatable spans).
    alternatives: ValueError unless None or all-empty (training on merged classes is not part of the pronunciation alternatives).
    return_pronunciation: ValueError if set (the pronunciation scores are read off an alignment; the loss has none to report)."""
    if repeat_spans is not None and any(len(v or ()) for v in repeat_spans):
        raise ValueError("anchored_alignment_loss: repeat_spans are not supported (no sum-product sweep on the lattice with repeatable spans)")
    if alternatives is not None and any(len(v or ()) for v in alternatives):
        raise ValueError("anchored_alignment_loss: alternatives are not supported (the loss is not defined on merged classes)")
    if return_pronunciation:
        raise ValueError("anchored_alignment_loss: return_pronunciation is not supported (the pronunciation scores belong to the aligner)")
    if on_infeasible not in ("raise", "skip"):
        raise ValueError('anchored_alignment_loss: on_infeasible must be "raise" or "skip"')
    if not torch.is_tensor(align_logit) or align_logit.dim() != 3 or not align_logit.is_cuda or align_logit.dtype != torch.float32:
        raise ValueError("anchored_alignment_loss: align_logit must be a float32 device tensor [B, T, V+1]")
    B, T, W = align_logit.shape
    if W < 4:
        raise ValueError("anchored_alignment_loss: align_logit needs the silence logit behind at least three word columns (the CTC variant)")
    dev = align_logit.device
    counts = [T] * B
    nf = None
    if n_frames is not None:
        counts = [int(v) for v in (n_frames.tolist() if torch.is_tensor(n_frames) else n_frames)]
        if len(counts) != B or any(v < 0 or v > T for v in counts):
            raise ValueError(f"n_frames: {B} frame counts in 0..{T} expected")
        nf = torch.tensor(counts, dtype=torch.int32).to(dev)
    lab, windows, skip = anchored_loss_inputs(labels, counts, onset_anchors, char_windows, optional_spans, hop_size_second)
    loss, _nll, status = _AnchoredAlignmentLoss.apply(align_logit, lab.to(dev), windows[0].to(dev), windows[1].to(dev), nf,
                                                      None if skip is None else skip.to(dev), float(skip_penalty), W - 1)
    if on_infeasible == "raise":
        raise_for_loss_status(status)
    return loss


def raise_for_loss_status(status) -> None:
    """status [B] of la_anchored_alignment_loss (reads it: a host synchronisation) -> ValueError naming the first clip that is not LA_OK."""
    for b, st in enumerate(status.tolist()):
        if st == LA_EINFEASIBLE:
            raise ValueError(f"anchored_alignment_loss: clip {b} has no alignment inside its windows (or too few frames for its labels)")
        if st == LA_EEMPTY:
            raise ValueError(f"anchored_alignment_loss: clip {b} has no labels")
        if st != LA_OK:
            raise ValueError(f"anchored_alignment_loss: clip {b}: status {int(st)}")


def run_viterbi_core(dp_matrix, backtrace_dp_matrix, cur_log_prediction, cur_log_silence_prediction, cur_label):
    """In place on the caller's numpy arrays and returned, like the reference (dp float64 [T,S], bt int64 [T,S],
    lp float32 [T,V'], ls float32 [T,1], label int64 [L]); row 0 of dp is taken as initialised by the caller."""
    dev = _device_of(None)
    lp = np.asarray(cur_log_prediction, dtype=np.float32)
    ls = np.asarray(cur_log_silence_prediction, dtype=np.float32).reshape(lp.shape[0], -1)[:, :1]
    label = np.asarray(cur_label, dtype=np.int64)
    T, L = lp.shape[0], label.shape[0]
    S = 2 * L + 1
    if dp_matrix.shape != (T, S) or backtrace_dp_matrix.shape != (T, S):
        raise ValueError("dp / backtrace matrices must be [T, 2L+1]")
    em = torch.from_numpy(np.ascontiguousarray(np.concatenate([ls, lp[:, label - 1]], axis=1))).to(dev)          # compact layout (gather = data movement)
    dp = torch.from_numpy(np.ascontiguousarray(dp_matrix, dtype=np.float64)).to(dev)
    bt = torch.from_numpy(np.ascontiguousarray(backtrace_dp_matrix, dtype=np.int64)).to(dev)
    lab = torch.from_numpy(label.astype(np.int32)).to(dev)
    nl = torch.tensor([L], dtype=torch.int32, device=dev)
    nf = torch.tensor([T], dtype=torch.int32, device=dev)
    scratch_i = torch.empty((2 * L + 1,), dtype=torch.int32, device=dev)
    scratch_f = torch.empty((1,), dtype=torch.float64, device=dev)
    need = ctypes.c_size_t(0)
    check(lib().la_viterbi_workspace_bytes(1, T, L, ctypes.byref(need)), "viterbi_workspace_bytes")
    ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev)
    check(lib().la_viterbi_core(ptr(em), em.stride(0), ptr(lab), L, T, ptr(nl), ptr(nf), ptr(dp), ptr(bt), ptr(scratch_i),
                                ptr(scratch_f), ptr(ws), need.value, stream_ptr()), "viterbi_core")
    dp_matrix[...] = dp.cpu().numpy()
    backtrace_dp_matrix[...] = bt.cpu().numpy()
    return dp_matrix, backtrace_dp_matrix


def get_mae(gt, predict):
    """Mean absolute onset/offset error over every character of the batch (:190-199).  A handful of Python-float
    operations on host lists: kept in Python float64 so the value is bit-identical to the reference's."""
    error = 0.0
    cnt = 0
    for i in range(len(gt)):
        for j in range(len(gt[i])):
            error = error + abs(gt[i][j][0] - predict[i][j][0]) + abs(gt[i][j][1] - predict[i][j][1])
            cnt = cnt + 2.0
    error = error / cnt
    return error
