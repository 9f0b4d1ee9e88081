"""Host side of the off-sheet slots (la_emissions_offsheet_columns; ops.offsheet_columns; utils.alignment._off_sheet_of; the `off_sheet` /
`off_sheet_penalty` / `return_off_sheet` keywords): what a slot does to an alignment, on the float64 restatement alone; the helper's
expanded rows, ids, spans and every remapping against the independent restatement tests/offsheet_reference.py; every refusal, raised
before a device is touched; the tail of align_labels with recorders in the kernels' place; the declaration and every argument error of
the C entry under its own name.  The numbers are tested on the GPU (tests/test_gpu_offsheet.py)."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import offsheet_reference as osr
import windows_reference as wr
from test_host_lattice_routes import B, T, VR, calls  # noqa: F401  (calls: the recorder fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 0.02


def _ua():
    from lyricalignment_amd.utils import alignment as ua
    return ua


# ---------------------------------------------------------------------------------------------------------------- semantics
# T = 63 frames, classes 1 .. 12, the sheet [1, 2, 3 | 4, 5] at 6 frames per character: silence 0..7, line one 7..25, an off-sheet passage
# of 15 frames (classes 7, 8, 9) at 25..40, line two 40..52, silence to the end.
SHEET, PASSAGE, FRAMES = [1, 2, 3, 4, 5], (25, 40), 63
TRUTH = [(7, 13), (13, 19), (19, 25), (40, 46), (46, 52)]


def _song():
    rs = np.random.RandomState(3)
    sung = np.zeros(FRAMES, dtype=np.int64)
    for c, (t, u) in zip(SHEET, TRUTH):
        sung[t:u] = c
    for k, c in enumerate((7, 8, 9)):
        sung[PASSAGE[0] + 5 * k: PASSAGE[0] + 5 * (k + 1)] = c
    logits = rs.normal(0.0, 0.3, size=(FRAMES, 13))
    logits[np.arange(FRAMES), sung] += np.where(sung > 0, 7.0, 0.0)
    silence = np.where(sung > 0, 1e-4, 0.97)
    return logits, silence


def _aligned(slots, penalty):
    """-> (largest boundary error in frames, the slot visits) of the float64 DP on the sheet with these slots."""
    logits, silence = _song()
    sheet = osr.Sheet(SHEET, slots)
    em = osr.write_columns(osr.ctc_emissions(logits, silence, sheet.expanded), sheet.slot_pos.values(), FRAMES, penalty)
    on, off, _, status, path = osr.viterbi(em, sheet.ids, sheet.skip_from())
    assert status == 0
    on, off = sheet.without_slots(on), sheet.without_slots(off)
    err = max(max(abs(a - t), abs(b - u)) for a, b, (t, u) in zip(on, off, TRUTH))
    return err, sheet.slot_visits(path)


def test_a_slot_takes_the_off_sheet_passage_and_without_it_a_character_is_stretched_over_it():
    err, visits = _aligned([], 0.0)
    print("largest boundary error without slots:", err)
    assert err >= 10 and visits == []
    for penalty in (math.log(10.0), math.log(100.0)):
        err, visits = _aligned([3], penalty)
        assert err == 0 and visits == [(3, *PASSAGE)], (penalty, err, visits)
        err, visits = _aligned([0, 3, 5], penalty)                 # the two edge slots are unused
        assert err == 0 and visits == [(3, *PASSAGE)], (penalty, err, visits)


def test_the_penalty_matters_at_zero_the_edge_slots_steal_frames():
    err, visits = _aligned([0, 3, 5], 0.0)
    print("largest boundary error at penalty 0:", err, visits)
    assert err > 0 and {n for n, _, _ in visits} == {0, 3, 5}


def test_the_column_formula():
    x = np.array([0.0, -6e-8, -1e-3, -0.69, -5.0, -50.0, -999.0, -1000.0, 0.5, np.nan], dtype=np.float32)
    got = osr.column(x, 0.0)
    assert got[0] == -1000.0 and got[8] == -1000.0 and got[9] == -1000.0          # log 0, log of a negative number, NaN: the floor
    for i in range(1, 8):
        want = math.log(-math.expm1(float(x[i])))
        assert abs(float(got[i]) - want) <= 2.0 ** -23 * max(1.0, abs(want))
    assert got[7] == 0.0 and got[5] == 0.0                                      # silence impossible: voiced for sure
    assert (osr.column(x, 2000.0) == -1000.0).all()
    assert osr.column(np.float32(-0.69), math.log(100.0)) == np.float32(math.log(-math.expm1(float(np.float32(-0.69)))) - math.log(100.0))


# ---------------------------------------------------------------------------------------------------------------- the host function
LISTS = [[3, 5, 5, 9, 4], [7, 7], [2]]
SLOTS = [[3, 0, 5], [1], []]


def test_the_helper_builds_expanded_rows_ids_spans_and_every_remapping():
    ua = _ua()
    spans = [[(3, 5), (0, 3), (1, 2)], [], [(0, 1)]]
    repeats = [[(0, 3), (3, 5)], [(0, 2)], None]
    anchors = [[(3, 1.0, 0.1), (0, 0.2, 0.1)], [(1, 0.5, 0.0)], []]
    windows = [[(4, None, 2.0)], [], [(0, 0.0, None)]]
    alts = [[(4, [9, 8]), (0, [1])], [(1, [2])], []]
    off = ua._off_sheet_of("t", SLOTS, 4.5, LISTS, spans, repeats, windows, anchors, alts)
    assert off.slots == [[0, 3, 5], [1], []] and off.penalty == 4.5 and off.n_slots.tolist() == [3, 1, 0]
    assert ua.OFF_SHEET_ID == osr.OFF_SHEET_ID == 1 << 25 and ua.OFF_SHEET_ID > ua.READING_SET_ID + 4095
    assert off.lattice_ids.dtype == torch.int32 and off.slot_cols.dtype == torch.int32 and off.lattice_ids.shape == (3, 8)
    for b, (labs, slots) in enumerate(zip(LISTS, SLOTS)):
        sheet = osr.Sheet(labs, slots)
        assert off.label_lists[b] == sheet.expanded and off.lattice_ids[b, : sheet.L].tolist() == sheet.ids
        assert off.slot_cols[b, : len(slots)].tolist() == [p for _, p in sorted(sheet.slot_pos.items())] and off.keep[b] == sheet.label_pos
        assert [tuple(s) for s in off.optional_spans[b]] == sheet.optional_spans(spans[b])
        assert off.n_caller_spans[b] == len(spans[b])
        assert [tuple(s) for s in off.repeat_spans[b]] == [sheet.span(a, e) for a, e in (repeats[b] or ())]
        assert [tuple(v) for v in off.onset_anchors[b]] == sheet.indexed(anchors[b])
        assert [tuple(v) for v in off.char_windows[b]] == sheet.indexed(windows[b])
        assert [(n, list(x)) for n, x in off.alternatives[b]] == [(n, list(x)) for n, x in sheet.indexed(alts[b])]
        # the product's own span and repeat rows on the expanded sheet are the restatement's
        assert ua._skip_from_of_spans(off.optional_spans, off.label_lists)[b, : sheet.L + 1].tolist() == sheet.skip_from(spans[b])
        assert ua._repeat_from_of_spans(off.repeat_spans, off.label_lists)[b, : sheet.L].tolist() == sheet.repeat_from(repeats[b] or ())
    # spelled out once: slots before labels 0, 3 and after the last of [3, 5, 5, 9, 4]
    assert off.label_lists[0] == [0, 3, 5, 5, 0, 9, 4, 0] and off.slot_cols[0].tolist() == [0, 4, 7]
    assert [tuple(s) for s in off.optional_spans[0]] == [(5, 7), (1, 4), (2, 3), (0, 1), (4, 5), (7, 8)]       # edge slots stay outside
    assert off.label_lists[1] == [7, 0, 7] and off.lattice_ids[1, :3].tolist() == [7, 1 << 25, 7]
    # a slot strictly inside a span belongs to it
    inside = ua._off_sheet_of("t", [[2]], 1.0, [[1, 2, 3, 4]], [[(1, 3)]], [[(0, 4)]])
    assert [tuple(s) for s in inside.optional_spans[0]] == [(1, 4), (2, 3)] and [tuple(s) for s in inside.repeat_spans[0]] == [(0, 5)]
    # keywords not given stay None; windows on L' states
    bare = ua._off_sheet_of("t", [[1]], 1.0, [[1, 2]])
    assert bare.repeat_spans is None and bare.char_windows is None and bare.onset_anchors is None and bare.alternatives is None
    assert [tuple(s) for s in bare.optional_spans[0]] == [(1, 2)] and bare.n_caller_spans == [0]
    anchored = ua._off_sheet_of("t", [[1]], 1.0, [[1, 2, 3]], onset_anchors=[[(2, 0.5, 0.1)]])
    lo, hi = ua._windows_of(None, anchored.onset_anchors, anchored.label_lists, [50], HOP)
    assert (lo.tolist(), hi.tolist()) == tuple([list(v)] for v in ua.windows_from_anchors(4, 50, None, [(3, 0.5, 0.1)], HOP))
    # the readings of the expanded sheet carry the slot id where the helper is told to
    rd = ua._readings_of(off.alternatives, off.label_lists)
    ids = off.ids_with_slots(rd.lattice_ids)
    assert ids[0, [0, 4, 7]].tolist() == [1 << 25] * 3 and ids[0, 1] >= ua.READING_SET_ID and ids[0, 2] == 5
    # the pronunciation candidates ignore the slots
    pron = ua._pronunciation_of("t", True, [6], 3, off.label_lists, None, off.slot_sets())
    assert pron.classes == [2, 3, 4, 5, 6, 7, 9] and pron.own_col[0].tolist() == [-1, 1, 3, 3, -1, 6, 2, -1]


def test_none_and_all_empty_return_none():
    ua = _ua()
    assert ua._off_sheet_of("t", None, 1.0, LISTS) is None
    assert ua._off_sheet_of("t", [[], [], []], 1.0, LISTS) is None and ua._off_sheet_of("t", [None, (), []], float("nan"), LISTS) is None


def test_every_refusal_of_the_helper():
    ua = _ua()
    lists = [[3, 5, 7], []]
    for bad in ([[1]],                                               # a wrong list count
                [[4], []], [[-1], []], [[1.5], []], [[float("nan")], []], [[True], []], [[None], []], [["1"], []], [[float("inf")], []],     # no integer in 0 .. L
                [[1, 1], []],                                        # a duplicate
                [[], [0]]):                                          # a slot on a clip without labels
        with pytest.raises(ValueError, match="off_sheet"):
            ua._off_sheet_of("t", bad, 1.0, lists)
    assert ua._off_sheet_of("t", [[0, 3], []], 1.0, lists).slots == [[0, 3], []]          # 0 and L are positions
    assert ua._off_sheet_of("t", [np.array([3, 0]), np.array([], dtype=np.int64)], 1.0, lists).slots == [[0, 3], []]      # array and tensor rows
    assert ua._off_sheet_of("t", [torch.tensor([2]), None], 1.0, lists).slots == [[2], []]
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="off_sheet_penalty"):
            ua._off_sheet_of("t", [[1], []], bad, lists)
    assert ua._off_sheet_of("t", [[1], []], 0.0, lists).penalty == 0.0
    wide = [list(range(1, 4095))]                                     # 4094 labels: one slot is taken, two are not
    assert len(ua._off_sheet_of("t", [[7]], 1.0, wide).label_lists[0]) == 4095
    with pytest.raises(NotImplementedError, match="4095"):
        ua._off_sheet_of("t", [[7, 9]], 1.0, wide)
    narrow = [list(range(1, 511))]                                    # 510 labels
    assert len(ua._off_sheet_of("t", [[7]], 1.0, narrow, narrow=True).label_lists[0]) == 511
    with pytest.raises(NotImplementedError, match="511"):
        ua._off_sheet_of("t", [[7, 9]], 1.0, narrow, narrow=True)
    assert len(ua._off_sheet_of("t", [[7, 9]], 1.0, narrow).label_lists[0]) == 512
    # an index the keyword's own check refuses stays refusable after the remapping
    off = ua._off_sheet_of("t", [[1], []], 1.0, lists, optional_spans=[[(1, 4)], []], onset_anchors=[[(3, 0.1, 0.1)], []],
                           alternatives=[[(-1, [2])], []])
    with pytest.raises(ValueError):
        ua._skip_from_of_spans(off.optional_spans, off.label_lists)
    with pytest.raises(ValueError):
        ua._windows_of(None, off.onset_anchors, off.label_lists, [50, 50], HOP)
    with pytest.raises(ValueError):
        ua._readings_of(off.alternatives, off.label_lists)


def test_the_public_functions_refuse_before_a_device_is_touched(monkeypatch):
    from lyricalignment_amd.harness import align_record_lines, align_record_lrc, align_song
    from lyricalignment_amd.module.align_model import AlignModel
    ua = _ua()
    monkeypatch.setattr(ua, "_device_of", lambda prediction: (_ for _ in ()).throw(AssertionError("a device was asked for")))
    logits, labels = torch.zeros((1, 20, 12)), torch.tensor([[3, 5, 7]])
    family = [getattr(ua, "perform_viterbi" + ctc + kind) for ctc in ("", "_ctc")
              for kind in ("", "_scored", "_anchored_scored", "_sheet_scored", "_repeat_scored", "_song_scored")]
    for f in family:
        sig = inspect.signature(f).parameters
        assert sig["off_sheet"].default is None and sig["off_sheet_penalty"].default == math.log(100) and sig["return_off_sheet"].default is False
        for bad in ([[4]], [[1, 1]], [[0.5]], [[], []]):
            with pytest.raises(ValueError, match="off_sheet"):
                f(logits, labels, off_sheet=bad)
        with pytest.raises(ValueError, match="off_sheet_penalty"):
            f(logits, labels, off_sheet=[[1]], off_sheet_penalty=-1.0)
        with pytest.raises(AssertionError, match="a device was asked for"):          # good slots go on to the device
            f(logits, labels, off_sheet=[[0, 3]])
    wide = torch.arange(1, 4096)[None]
    with pytest.raises(NotImplementedError):
        ua.perform_viterbi(logits, wide, off_sheet=[[0]])
    with pytest.raises(NotImplementedError):
        ua.perform_viterbi_scored(logits, torch.arange(1, 512)[None], off_sheet=[[0]])
    with pytest.raises(AssertionError):                                                # the sheet kind takes whole songs
        ua.perform_viterbi_sheet_scored(logits, torch.arange(1, 512)[None], off_sheet=[[0]])

    class Unbuilt(AlignModel):                                          # align's keyword checks come before the engine exists
        def __init__(self):
            pass

        def engine(self):
            raise AssertionError("the refusal comes before anything is on a device")

    audio = [np.zeros(16000, np.float32)]
    for bad in ([[4]], [[1, 1]], [[0.5]], [[], []]):
        with pytest.raises(ValueError, match="off_sheet"):
            AlignModel.align(Unbuilt(), audio, labels, off_sheet=bad)
    with pytest.raises(ValueError, match="off_sheet_penalty"):
        AlignModel.align(Unbuilt(), audio, labels, off_sheet=[[1]], off_sheet_penalty=float("nan"))
    with pytest.raises(ValueError, match="return_confidence is not defined with off_sheet"):
        AlignModel.align(Unbuilt(), audio, labels, off_sheet=[[1]], return_confidence=True)
    with pytest.raises(ValueError, match="return_frames"):
        AlignModel.align(Unbuilt(), audio, labels, off_sheet=[[1]], return_frames=True)
    with pytest.raises(NotImplementedError):
        AlignModel.align(Unbuilt(), audio, wide, off_sheet=[[0]])
    with pytest.raises(NotImplementedError):
        AlignModel.align(Unbuilt(), audio, torch.arange(1, 512)[None], off_sheet=[[0]], return_span_confidence=True)
    with pytest.raises(AssertionError):
        AlignModel.align(Unbuilt(), audio, torch.arange(1, 512)[None], off_sheet=[[0]], return_sheet_confidence=True)
    with pytest.raises(AssertionError):                                 # good slots are accepted (and go on to the engine)
        AlignModel.align(Unbuilt(), audio, labels, off_sheet=[[0, 3]], return_off_sheet=True)
    sig = inspect.signature(AlignModel.align).parameters
    assert sig["off_sheet"].default is None and sig["off_sheet_penalty"].default == math.log(100) and sig["return_off_sheet"].default is False
    assert "off_sheet" in AlignModel.align.__doc__ and "NOT BEEN TUNED" in AlignModel.align.__doc__
    for f in (align_record_lines, align_record_lrc, align_song):
        sig = inspect.signature(f).parameters
        assert sig["off_sheet"].default is False and sig["off_sheet_penalty"].default == math.log(100)


# ---------------------------------------------------------------------------------------------------------------- the tail
@pytest.fixture
def column_calls(monkeypatch):
    from lyricalignment_amd import ops
    log = []

    def offsheet_columns(em, slot_cols, n_slots, n_frames, penalty):
        log.append((em, slot_cols, n_slots, n_frames, penalty))
        return em
    monkeypatch.setattr(ops, "offsheet_columns", offsheet_columns)
    return log


class _Emissions:
    def __init__(self, fused=False):
        self.asked, self.fused = [], fused

    def __call__(self, lab, n_lab, needed=True):
        self.asked.append((lab, n_lab, needed))
        dp = (torch.full(lab.shape, 4, dtype=torch.int32), torch.full(lab.shape, 5, dtype=torch.int32), torch.zeros((B,), dtype=torch.float64),
              torch.zeros((B,), dtype=torch.int32))
        return (dp if self.fused else None), torch.zeros((B, T, lab.shape[1] + 1)) if needed or not self.fused else None


TAIL_LISTS = [[3, 5, 3], [4, 6]]


def _tail(emissions_of, off_sheet, confidence=None, return_segments=False, optional_spans=None, repeat_spans=None, return_off_sheet=True):
    ua = _ua()
    off = ua._off_sheet_of("t", off_sheet, 2.5, TAIL_LISTS, optional_spans, repeat_spans)
    lists = TAIL_LISTS if off is None else off.label_lists
    spans = optional_spans if off is None else off.optional_spans
    lab, n_lab, lists = ua._labels_to_device(lists, B, torch.device("cpu"))
    skip_from = ua._skip_from_of_spans(spans, lists)
    return ua.align_labels("perform_viterbi", emissions_of, lab, n_lab, lists, [T] * B, T, None, HOP, confidence, 2, skip_from, None, 0.0, spans,
                           repeat_spans if off is None else off.repeat_spans, 0.0, return_segments, None, False, off=off,
                           return_off_sheet=return_off_sheet), off, lab


def test_the_tail_writes_the_columns_once_runs_the_expanded_lattice_and_drops_the_slots(calls, column_calls):  # noqa: F811
    emissions_of = _Emissions(fused=True)
    (seconds, heard), off, lab = _tail(emissions_of, [[0, 2], [2]])
    # the provider: once, for the expanded rows, emissions needed; its own DP result is dropped
    assert len(emissions_of.asked) == 1 and emissions_of.asked[0][0] is lab and emissions_of.asked[0][2] is True
    assert lab.tolist() == [[0, 3, 5, 0, 3], [4, 6, 0, 0, 0]]
    # the kernel: once, on the matrix the lattice reads, before it
    assert len(column_calls) == 1 and column_calls[0][0] is calls[0][1]["em"] and column_calls[0][4] == 2.5
    assert column_calls[0][1].tolist() == [[0, 3], [2, -1]] and column_calls[0][2].tolist() == [2, 1] and column_calls[0][3].tolist() == [T, T]
    # the lattice: the span DP on L' labels with the slot ids, each slot a one-label span
    assert [c[0] for c in calls] == ["viterbi_spans_batch"]
    assert calls[0][1]["labels"].tolist() == [[1 << 25, 3, 5, 1 << 25, 3], [4, 6, 1 << 25, 0, 0]]
    assert calls[0][1]["skip_from"].tolist() == [[-1, 0, -1, -1, 3, -1], [-1, -1, -1, 2, -1, -1]]
    # the way out: the caller's characters, and the recorder's frames 0 .. 1 for every slot
    assert seconds == [[[0.0, HOP]] * 3, [[0.0, HOP]] * 2]
    assert heard == [[{"position": 0, "onset": 0.0, "offset": HOP, "frames": 1}, {"position": 2, "onset": 0.0, "offset": HOP, "frames": 1}],
                     [{"position": 2, "onset": 0.0, "offset": HOP, "frames": 1}]]


def test_the_tail_with_confidences_and_segments(calls, column_calls):  # noqa: F811
    # a span confidence: per-character lists lose the slots, span_skip_prob keeps the caller's spans, off_sheet_prob names every slot
    (seconds, scores, heard), off, _ = _tail(_Emissions(), [[0, 2], [2]], confidence="sheet", optional_spans=[[(1, 3)], []])
    assert calls[0][1]["skip_from"].tolist() == [[-1, 0, -1, -1, 3, 2], [-1, -1, -1, 2, -1, -1]]
    assert [len(d["occupancy"]) for d in scores] == [3, 2] and [len(d["sung_prob"]) for d in scores] == [3, 2]
    assert [len(d["span_skip_prob"]) for d in scores] == [1, 0]
    assert [d["off_sheet_prob"] for d in scores] == [{0: 0.0, 2: 0.0}, {2: 0.0}]
    # a repeat kind with segments: the recorder's path sits in state 1 -- clip 0: the slot before label 0, clip 1: label 0
    del calls[:]
    (seconds, segments, scores, heard), off, _ = _tail(_Emissions(), [[0, 2], [2]], confidence="song", return_segments=True, repeat_spans=[[(0, 2)], []])
    assert calls[0][0] == VR and calls[0][1]["repeat_from"].tolist() == [[-1, 3, -1, -1, -1], [-1] * 5]       # labels 0 .. 1 sit at 1 .. 2
    assert segments == [[], [(0, 0.0, T * HOP)]]
    assert heard == [[{"position": 0, "onset": 0.0, "offset": T * HOP, "frames": T}], []]
    assert scores[0]["visit_occupancy"] == [] and len(scores[1]["visit_occupancy"]) == 1
    assert list(scores[0]["repeat_count"]) == [(0, 2)] and scores[0]["off_sheet_prob"] == {0: 0.0, 2: 0.0} and len(scores[0]["visits"]) == 3
    # segments without a confidence go back to the caller's numbering too
    del calls[:]
    (seconds, segments, heard), _, _ = _tail(_Emissions(), [[], [0]], return_segments=True)
    assert segments == [[(0, 0.0, T * HOP)], []] and heard == [[], [{"position": 0, "onset": 0.0, "offset": T * HOP, "frames": T}]]


def test_repeat_count_goes_back_to_the_callers_spans_key_by_key():
    ua = _ua()
    off = ua._off_sheet_of("t", [[0, 3], []], 1.0, [[1, 2, 3, 4, 5], [7]], repeat_spans=[[(2, 5), (0, 2)], []])
    assert [tuple(v) for v in off.repeat_spans[0]] == [(3, 7), (1, 3)]
    scores = [{"repeat_count": {(1, 3): 0.25, (3, 7): 0.5}, "visits": [0.0] * 7}, {"repeat_count": {}, "visits": [1.0]}]      # another order than given
    out = ua._scores_without_slots(off, scores)
    assert out[0]["repeat_count"] == {(0, 2): 0.25, (2, 5): 0.5} and out[1]["repeat_count"] == {} and len(out[0]["visits"]) == 5


class _StubModel:
    """Answers AlignModel.align's return for one clip of two lines (2 + 2 characters) from what the keywords ask for, in align's order:
    seconds [, segments] [, scores] [, readings] [, pronunciation] [, off_sheet]."""

    def align(self, audios, labels, **kw):
        self.kw = kw
        out = [[[[0.1 * n, 0.1 * n + 0.1] for n in range(4)]]]
        if kw.get("return_segments"):
            out.append([[(n, 0.1 * n, 0.1 * n + 0.1) for n in range(4)]])
        if any(kw.get(k) for k in ("return_span_confidence", "return_anchored_confidence", "return_sheet_confidence", "return_song_confidence")):
            d = {"sung_prob": [1.0] * 4, "onset_prob": [0.5] * 4, "window_log_prob": 0.0, "occupancy": [1.0] * 4, "visits": [1.0] * 4,
                 "repeat_count": {(2, 4): 0.0}, "visit_occupancy": [1.0] * 4}
            if "off_sheet" in kw:
                d["off_sheet_prob"] = {n: 0.9 - 0.1 * i for i, n in enumerate(kw["off_sheet"][0])}
            out.append([d])
        if kw.get("return_readings"):
            out.append([[(int(c), [0.0]) for c in labels[0]]])
        if kw.get("return_pronunciation"):
            out.append([[{"class": int(c), "frames": 5, "log_prob": -0.1, "rank": 0, "gop": 0.0, "top": [(int(c), -0.1)]} for c in labels[0]]])
        if kw.get("return_off_sheet"):
            out.append([[{"position": 2, "onset": 0.25, "offset": 0.3, "frames": 2, **({"top": [(3, -0.5)]} if kw.get("return_pronunciation") else {})}]])
        return out[0] if len(out) == 1 else tuple(out)


def test_the_sheet_functions_return_passages_and_off_sheet_prob_whatever_else_is_asked_for():
    from lyricalignment_amd.harness import PinyinClassLUT, align_record_lines, align_record_lrc, align_song
    syllables = ["sil", "a", "bo", "ci", "de", "e"]
    lut = PinyinClassLUT(syllables, {s: i for i, s in enumerate(syllables)})
    lines, ids = ["一二", "三四"], {"一二": [4, 3], "三四": [1, 2]}
    tok = lambda t: ids[t]
    passages, prob = [(1, 0.25, 0.3)], {0: 0.9, 1: 0.8, 2: 0.7}
    heard = [(1, 0.25, 0.3, [("ci", -0.5)])]
    model = _StubModel()
    base = align_record_lines(model, None, lines, [False, False], lut, tok)
    assert "off_sheet" not in model.kw and "return_off_sheet" not in model.kw                       # off: the call as it was
    assert align_record_lines(model, None, lines, [False, False], lut, tok, off_sheet=False) == base and "off_sheet" not in model.kw
    assert align_record_lines(model, None, lines, [False, False], lut, tok, off_sheet=[]) == base and "off_sheet" not in model.kw
    got = align_record_lines(model, None, lines, [False, False], lut, tok, off_sheet=True, off_sheet_penalty=3.0)
    assert got == (base, passages) and model.kw["off_sheet"] == [[0, 2, 4]] and model.kw["off_sheet_penalty"] == 3.0 and model.kw["return_off_sheet"]
    assert align_record_lines(model, None, lines, [False, False], lut, tok, off_sheet=[1]) == (base, passages) and model.kw["off_sheet"] == [[2]]
    for f, args, conf_kw in ((align_record_lines, (lines, [False, False]), dict(with_confidence=True)),
                             (align_record_lrc, ([(0.0, lines[0]), (0.2, lines[1])],), dict(with_confidence=True)),
                             (align_song, (lines,), dict()),
                             (align_song, (lines,), dict(repeatable=[False, True]))):
        plain = f(model, None, *args, lut, tok, **conf_kw)
        for extra, tail in ((dict(), (passages, prob)), (dict(with_pronunciation=True), (heard, prob)), (dict(heteronyms={4: ["e"]}), (passages, prob)),
                            (dict(with_pronunciation=True, heteronyms={4: ["e"]}), (heard, prob))):
            without = f(model, None, *args, lut, tok, **conf_kw, **extra)
            out = f(model, None, *args, lut, tok, off_sheet=True, **conf_kw, **extra)
            want = without if "with_pronunciation" in extra else (without,)          # (result, pronunciation) already is a tuple
            assert isinstance(out, tuple) and out == (*want, *tail), (f.__name__, conf_kw, extra, out)
        assert f(model, None, *args, lut, tok, off_sheet=False, **conf_kw) == plain
    # without a confidence option there is no probability to report, with pronunciation or without
    out = align_record_lrc(model, None, [(0.0, lines[0]), (0.2, lines[1])], lut, tok, off_sheet=True, with_pronunciation=True)
    assert len(out) == 3 and out[2] == heard


def test_none_and_all_empty_never_reach_the_kernel(calls, monkeypatch):  # noqa: F811
    from lyricalignment_amd import ops
    ua = _ua()
    monkeypatch.setattr(ops, "offsheet_columns", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the kernel was reached")))
    for off_sheet in (None, [[], []], [None, ()]):
        emissions_of = _Emissions(fused=True)
        (seconds, heard), off, lab = _tail(emissions_of, off_sheet)
        assert off is None and calls == [] and emissions_of.asked[0][2] is False          # the fused shortcut: the call as it was
        assert seconds == [[[4 * HOP, 5 * HOP]] * 3, [[4 * HOP, 5 * HOP]] * 2] and heard == [[], []]
        out, _, _ = _tail(_Emissions(fused=True), off_sheet, return_off_sheet=False)
        assert out == seconds
    # and the public function hands the tail the caller's own sheet
    seen = {}
    monkeypatch.setattr(ua, "_device_of", lambda prediction: torch.device("cpu"))
    monkeypatch.setattr(ua, "align_labels", lambda *a, **k: seen.update(a=a, k=k))
    labels = torch.tensor([[3, 5, 3], [4, 6, -100]])
    ua.perform_viterbi(torch.zeros((2, T, 12)), labels, off_sheet=[[], []], optional_spans=[[(0, 1)], []])
    assert seen["k"]["off"] is None and seen["a"][4] == TAIL_LISTS and seen["a"][14] == [[(0, 1)], []]
    ua.perform_viterbi(torch.zeros((2, T, 12)), labels, off_sheet=[[1], []], optional_spans=[[(0, 1)], []])
    assert seen["k"]["off"].slots == [[1], []] and seen["a"][4] == [[3, 0, 5, 3], [4, 6]] and seen["a"][14] == [[(0, 1), (1, 2)], [()] * 0]


# ---------------------------------------------------------------------------------------------------------------- the C entry
def test_the_entry_point_is_declared_and_exported():
    from lyricalignment_amd import _lib, ops
    name = "la_emissions_offsheet_columns"
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lyricalign.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert decl, f"{name} not declared in lyricalign.h"
    assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == decl.group(1).count(",") + 1 == 13
    assert _lib.SYMBOLS[name][1][11] is ctypes.c_double
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} not exported"
    assert callable(ops.offsheet_columns)


def test_every_argument_error_is_answered_on_the_host_under_the_entrys_name():
    from lyricalignment_amd import _lib
    L = _lib.lib()
    P = 16                                      # a non-null stand-in pointer: every call below is refused before any device call
    frames, labels, slots = 100, 29, 3

    def call(em=P, ebs=None, ers=labels + 1, slot_cols=P, slot_stride=slots, n_slots=P, n_frames=P, batch=2, T=frames, Lmax=labels, S=slots,
             penalty=4.6):
        return L.la_emissions_offsheet_columns(em, frames * ers if ebs is None else ebs, ers, slot_cols, slot_stride, n_slots, n_frames, batch,
                                               T, Lmax, S, penalty, 0)

    def refused(what, rc=_lib.LA_EINVAL, **kw):
        assert call(**kw) == rc, kw
        assert what in _lib.last_error() and "emissions_offsheet_columns" in _lib.last_error(), (kw, _lib.last_error())

    for null in ("em", "slot_cols", "n_slots", "n_frames"):
        refused("null", **{null: 0})
    for size in ("batch", "T", "Lmax", "S"):
        refused("sizes", **{size: 0})
        refused("sizes", **{size: -1})
    refused("penalty", penalty=-1e-9)
    refused("penalty", penalty=float("nan"))
    refused("strides", ers=labels)
    refused("strides", slot_stride=slots - 1)
    refused("4095", rc=_lib.LA_EUNSUPPORTED, Lmax=4096, ers=1)          # the limit: reported before the strides
