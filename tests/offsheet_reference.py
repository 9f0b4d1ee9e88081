"""tests/offsheet_reference.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Yardstick of the off-sheet slots (include/lyricalign.h la_emissions_offsheet_columns; utils.alignment._off_sheet_of): the column formula
in numpy float64, the expansion of a sheet by its slots and the remapping of the caller's keywords -- written independently of the
product code, position by position --, and a driver that runs the existing float64 restatements of the lattice
(windows_reference / repeat_spans_reference and the posterior yardsticks) on the expanded sheet.
"""
from __future__ import annotations

import numpy as np

import repeat_spans_reference as rr
import windows_reference as wr

FLOOR = -1000.0
OFF_SHEET_ID = 1 << 25


def column64(silence, penalty):
    """log P(frame is not silence) - penalty in float64 for float32 silence log-probabilities; NaN / -inf / silence >= 0 stay as they
    come out (floor32 maps them)."""
    x = np.asarray(silence, dtype=np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(-np.expm1(x)) - float(penalty)


def column(silence, penalty):
    """The slot's emission as the kernel defines it: the float64 value rounded once, the floor where it is not above -1000."""
    v = column64(silence, penalty)
    return np.where(v > FLOOR, v, FLOOR).astype(np.float32)          # NaN > x is False: the floor


def write_columns(em, slot_cols, n_frames, penalty):
    """One clip: em [T, >= 1 + L'] float32 -> a copy with column 1 + x of every slot x filled for the rows t < n_frames."""
    out = np.array(em, dtype=np.float32, copy=True)
    T = int(n_frames)
    val = column(out[:T, 0], penalty)
    for x in slot_cols:
        out[:T, 1 + int(x)] = val
    return out


def adjacent_or_equal(a, b):
    """float32 arrays: every pair equal or neighbours in float32 (one step of np.nextafter)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a == b) | (np.nextafter(a, b) == b)


class Sheet:
    """One clip's sheet with slots, walked position by position: slot n (if given) is emitted in front of label n, slot L after the last."""

    def __init__(self, labels, slots):
        self.labels = [int(c) for c in labels]
        self.slots = sorted(int(n) for n in slots)
        self.expanded, self.ids, self.slot_pos, self.label_pos = [], [], {}, []
        for n in range(len(self.labels) + 1):
            if n in self.slots:
                self.slot_pos[n] = len(self.expanded)
                self.expanded.append(0)
                self.ids.append(OFF_SHEET_ID)
            if n < len(self.labels):
                self.label_pos.append(len(self.expanded))
                self.expanded.append(self.labels[n])
                self.ids.append(self.labels[n])
        self.L = len(self.expanded)

    def span(self, a, e):
        """Labels a .. e-1 of the caller -> the expanded half-open range from label a's place to behind label e-1's: slots strictly inside
        come along, the slots before a and before e stay outside."""
        return self.label_pos[a], self.label_pos[e - 1] + 1

    def optional_spans(self, spans=()):
        """-> the caller's spans remapped, then one one-label span per slot in ascending position."""
        return [self.span(a, e) for a, e in spans] + [(p, p + 1) for _, p in sorted(self.slot_pos.items())]

    def skip_from(self, spans=()):
        row = [-1] * (self.L + 1)
        for a, e in self.optional_spans(spans):
            assert row[e] < 0, "two spans with one end"
            row[e] = a
        return row

    def repeat_from(self, spans=()):
        row = [-1] * self.L
        for a, e in spans:
            a, e = self.span(a, e)
            assert row[a] < 0, "two spans with one start"
            row[a] = e
        return row

    def indexed(self, items):
        """[(n, ...)] in the caller's numbering (anchors, windows, alternatives) -> the same with expanded positions."""
        return [(self.label_pos[item[0]], *item[1:]) for item in items]

    def without_slots(self, row):
        return [row[p] for p in self.label_pos]

    def slot_visits(self, path):
        """-> the time-ordered [(n, first frame, last frame + 1)] of the slot visits of a lattice path."""
        at = {p: n for n, p in self.slot_pos.items()}
        return [(at[p], t, u) for p, t, u in rr.segments(path) if p in at]


def viterbi(em, ids, skip_from, penalty=0.0, lo=None, hi=None, repeat_from=None, repeat_penalty=0.0):
    """The existing float64 restatements on the expanded lattice (ids in the labels' place) -> (onset, offset, score, status, path):
    repeat_spans_reference.viterbi where a repeat_from is given, else windows_reference.viterbi_windows (open windows without lo / hi)."""
    L, T = len(ids), len(em)
    if repeat_from is not None:
        return rr.viterbi(em, ids, skip_from, penalty, repeat_from, repeat_penalty, lo, hi, rows=True)
    if lo is None:
        lo, hi = wr.open_windows(L, T)
    return wr.viterbi_windows(em, ids, lo, hi, skip_from, penalty, rows=True)


def ctc_emissions(logits, silence_prob, labels):
    """The CTC variant's compact matrix in float64, rounded to float32: column 0 log P(silence), column 1 + n log softmax(logits)[class
    of label n] + log P(voiced); class 0 (a slot) gets the floor.  logits [T, C+1] with column c the logit of class c (column 0 unused)."""
    lg = np.asarray(logits, np.float64)[:, 1:]
    logp = lg - lg.max(1, keepdims=True)
    logp = logp - np.log(np.exp(logp).sum(1, keepdims=True))
    sil = np.asarray(silence_prob, np.float64)
    em = np.full((lg.shape[0], 1 + len(labels)), FLOOR)
    em[:, 0] = np.maximum(np.log(sil), FLOOR)
    for n, c in enumerate(labels):
        if c >= 1:
            em[:, 1 + n] = np.maximum(logp[:, c - 1] + np.log1p(-sil), FLOOR)
    return em.astype(np.float32)
