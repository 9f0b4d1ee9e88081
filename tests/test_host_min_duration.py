"""CPU-only checks of the alignment DP with a minimum character duration: the float64 restatement (tests/min_duration_reference.py)
against exhaustive enumeration of the valid paths and, with every floor 1, against tests/optional_spans_reference.py without spans; the
planted clip the feature exists for; _min_frames_of; every refusal of the Python surface with the device stubbed; keyword positions; the
host face of la_viterbi_min_duration_batch (declared, exported, argument checks answered before any device call) and the harness on a
stubbed align."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import min_duration_reference as md
import optional_spans_reference as osr
from conftest import ROOT


# ------------------------------------------------------------------------------------------------ 1. exhaustive enumeration
def test_the_restatement_equals_exhaustive_enumeration():
    """Random lattices of up to 3 labels x 10 frames over two classes with floors 1 .. 3: the DP's score is the maximum over ALL paths that
    keep every floor (the last visit included), accumulated in the same order; where no such path exists the status says so."""
    rs = np.random.RandomState(0)
    feasible = infeasible = changed = equal_neighbours = 0
    for case in range(300):
        L, T = int(rs.randint(1, 4)), int(rs.randint(1, 11))
        labels = [int(v) for v in rs.randint(1, 3, size=L)]
        floors = [int(v) for v in rs.randint(1, 4, size=L)]
        em = np.log(rs.dirichlet(np.ones(L + 1), size=T)).astype(np.float32)
        got = md.viterbi(em, labels, floors)
        want = md.enumerate_best(em, labels, floors)
        if want is None:
            assert got[3] == md.LA_EINFEASIBLE and got[0] == [-1] * L and got[1] == [-1] * L and got[4] == [], (case, got)
            infeasible += 1
            continue
        assert got[3] == md.LA_OK and got[2] == want, (case, labels, floors, T, got[2], want)
        assert all(b - a >= d for a, b, d in zip(got[0], got[1], floors)) and len(got[4]) == T
        assert got[0] == [got[4].index(2 * n + 1) for n in range(L)]
        assert got[1] == [T - got[4][::-1].index(2 * n + 1) for n in range(L)]
        feasible += 1
        changed += got[4] != md.plain(em, labels)[4]
        equal_neighbours += any(a == b for a, b in zip(labels, labels[1:]))
    assert feasible >= 150 and infeasible >= 50 and changed >= 50 and equal_neighbours >= 50, (feasible, infeasible, changed, equal_neighbours)


# ------------------------------------------------------------------------------------------------ 2. every floor 1: the plain lattice
def test_with_every_floor_one_it_is_the_plain_lattice():
    rs = np.random.RandomState(1)
    kinds = {"ok": 0, "infeasible": 0, "flat": 0, "equal": 0}
    for case in range(200):
        L, T = int(rs.randint(1, 10)), int(rs.randint(1, 40))
        labels = [int(v) for v in rs.randint(1, 4, size=L)]
        em = np.log(rs.dirichlet(np.ones(L + 1), size=T)).astype(np.float32)
        if case % 5 == 0:
            em[:] = -1.0                                                           # all-equal emissions: every comparison is a tie
            kinds["flat"] += 1
        kinds["equal"] += any(a == b for a, b in zip(labels, labels[1:]))
        got = md.plain(em, labels)
        want = osr.viterbi_spans(em, labels, [-1] * (L + 1), 0.0)
        if want[3] == md.LA_OK:
            assert tuple(got) == tuple(want), case
            kinds["ok"] += 1
        else:                                                                      # (the plain entry leaves partial rows there)
            assert got[3] == want[3] == md.LA_EINFEASIBLE and got[2] == want[2] and got[0] == [-1] * L and got[4] == [], case
            kinds["infeasible"] += 1
    assert all(v >= 20 for v in kinds.values()), kinds


def test_results_for_empty_and_invalid_clips():
    em = np.zeros((4, 3), dtype=np.float32)
    assert md.viterbi(em, [], []) == ([], [], 0.0, md.LA_EEMPTY, [])
    for bad in ([0, 1], [1, 9], [1]):
        assert md.viterbi(em, [1, 2], bad) == ([-1, -1], [-1, -1], 0.0, md.LA_EINVAL, [])


# ------------------------------------------------------------------------------------------------ 3. the case the feature exists for
def test_weak_tails_get_one_frame_on_the_plain_lattice_and_their_floor_with_it():
    """60 labels x 6 frames, floors up to 6 frames (never more than was sung): the plain lattice keeps the previous character through
    every weak tail and gives that character one frame."""
    c = md.weak_tail(3, 60, 420, seg=6, max_floor=6)
    assert max(c["floors"]) <= 6 and sum(c["weak"]) >= 20
    plain, floored = md.plain(c["em"], c["lab"]), md.viterbi(c["em"], c["lab"], c["floors"])
    assert plain[3] == md.LA_OK and floored[3] == md.LA_OK
    short = md.short_of_floor(plain[0], plain[1], c["floors"])
    assert 4 * short >= 60, short
    assert all(plain[1][n] - plain[0][n] == 1 for n in range(60) if c["weak"][n])
    assert md.short_of_floor(floored[0], floored[1], c["floors"]) == 0
    assert md.boundary_error(floored[0], floored[1], c) < md.boundary_error(plain[0], plain[1], c)
    assert floored[2] < plain[2]                                                   # a constraint never raises the best score


# ------------------------------------------------------------------------------------------------ 4. seconds -> frames
def test_min_frames_of():
    from lyricalignment_amd.utils.alignment import MIN_DURATION_MAX_FRAMES, _min_frames_of
    lists = [[1, 2, 3], [4], []]
    assert MIN_DURATION_MAX_FRAMES == 8
    assert _min_frames_of("f", None, lists, 0.02) is None
    for one_frame in (0.0, 0.01, 0.02, [[0.02, 0.0, 0.01], None, []], [None, None, None]):
        assert _min_frames_of("f", one_frame, lists, 0.02) is None                 # the call as it was
    rows = _min_frames_of("f", 0.04, lists, 0.02)
    assert rows.tolist() == [[2, 2, 2], [2, 1, 1], [1, 1, 1]] and str(rows.dtype) == "torch.int32" and not rows.is_cuda
    assert _min_frames_of("f", 0.0401, lists, 0.02).tolist()[0] == [3, 3, 3]
    assert _min_frames_of("f", 0.06, lists, 0.02).tolist()[0] == [3, 3, 3]         # 0.06 / 0.02 = 3.0000000000000004 in float64
    assert _min_frames_of("f", 0.16, lists, 0.02).tolist()[1] == [8, 1, 1]
    assert _min_frames_of("f", np.float32(0.04), lists, 0.02).tolist()[0] == [2, 2, 2]
    assert _min_frames_of("f", 0.04, lists, 0.01).tolist()[0] == [4, 4, 4]
    assert _min_frames_of("f", [[0.05, 0.0, 0.16], None, []], lists, 0.02).tolist() == [[3, 1, 8], [1, 1, 1], [1, 1, 1]]
    assert _min_frames_of("f", [None, [0.03], None], lists, 0.02).tolist() == [[1, 1, 1], [2, 1, 1], [1, 1, 1]]
    for bad in (-0.01, float("nan"), float("inf"), 0.1601, 1.0, "0.04", True, [[0.04] * 3, [0.04]], [[0.04] * 2, None, None],
                [[0.04] * 3, [0.2], []], [[0.04, -1.0, 0.0], None, None], [0.04, 0.04, 0.04], [[0.04, float("nan"), 0.0], None, None]):
        with pytest.raises(ValueError, match="min_duration"):
            _min_frames_of("f", bad, lists, 0.02)


# ------------------------------------------------------------------------------------------------ 5. refusals, before a device is asked for
class _Stop(Exception):
    pass


REFUSED = dict(optional_spans=[[(0, 1)]], repeat_spans=[[(0, 2)]], onset_anchors=[[(0, 0.1, 0.1)]], char_windows=[[(0, 0.0, 0.2)]],
               line_starts=[[0, 2]], off_sheet=[[1]])
CONFIDENCES = ("return_confidence", "return_span_confidence", "return_anchored_confidence", "return_sheet_confidence",
               "return_repeat_confidence", "return_song_confidence", "return_line_confidence")


def test_bad_values_and_every_refusal_come_before_a_device_is_asked_for(monkeypatch):
    from lyricalignment_amd import ops
    from lyricalignment_amd.module.align_model import AlignModel
    from lyricalignment_amd.utils import alignment as ua
    logits = torch.zeros((1, 20, 12))
    labels = torch.tensor([[3, 5, 7]])

    def launch(*a, **k):
        raise _Stop()

    monkeypatch.setattr(ua, "_device_of", launch)
    monkeypatch.setattr(ops, "emissions_from_logits", launch)
    monkeypatch.setattr(ops, "viterbi_min_duration_batch", launch)

    class Unbuilt(AlignModel):                                          # align's keyword checks come before the engine exists
        def __init__(self):
            pass

        def engine(self):
            raise _Stop()

    audio = [np.zeros(16000, np.float32)]
    calls = [lambda **kw: f(logits, labels, **kw) for f in (ua.perform_viterbi, ua.perform_viterbi_ctc)]
    calls.append(lambda **kw: AlignModel.align(Unbuilt(), audio, labels, **kw))
    for call in calls:
        for bad in (-0.1, float("nan"), 0.17, [[0.04]], [[0.04] * 3, None], [[0.04, 0.04, 0.2]]):
            with pytest.raises(ValueError, match="min_duration"):
                call(min_duration=bad)
        for name, value in REFUSED.items():
            with pytest.raises(ValueError, match=rf"min_duration.*{name}"):
                call(min_duration=0.06, **{name: value})
            with pytest.raises(ValueError, match=rf"min_duration.*{name}"):        # refused for being given, whatever the floor comes to
                call(min_duration=0.01, **{name: value})
        with pytest.raises(_Stop):                                      # good keywords are accepted (and go on to the device)
            call(min_duration=0.06, return_segments=True)
        with pytest.raises(_Stop):
            call(min_duration=[[0.06, 0.0, 0.16]], alternatives=[[(1, [4, 6])]], return_readings=True)
        with pytest.raises(_Stop):
            call(min_duration=0.06, return_pronunciation=True, pronunciation_classes=11)
        with pytest.raises(_Stop):                                      # all-empty companions are "not given"
            call(min_duration=0.06, optional_spans=[[]], off_sheet=[[]], repeat_spans=[[]])
    for name in CONFIDENCES:
        kw = dict(line_starts=[[0, 2]]) if name == "return_line_confidence" else {}
        with pytest.raises(ValueError, match=r"min_duration"):
            AlignModel.align(Unbuilt(), audio, labels, min_duration=0.06, **{name: True}, **kw)
    with pytest.raises(ValueError, match=r"min_duration.*return_confidence"):
        AlignModel.align(Unbuilt(), audio, labels, min_duration=0.06, return_confidence=True)
    # the _scored functions, the line-confidence functions and the training entries do not have the keyword
    for name in dir(ua):
        if name.endswith(("_scored", "_line_confidence")) or name in ("anchored_alignment_loss", "anchored_loss_inputs"):
            assert "min_duration" not in inspect.signature(getattr(ua, name)).parameters, name


def test_align_labels_sends_floors_to_the_new_entry_and_refuses_the_rest(monkeypatch):
    from lyricalignment_amd import ops
    from lyricalignment_amd.utils import alignment as ua
    seen = []

    def entry(em, lab, n_lab, nf, min_frames, max_min_frames=None, want_path=True):
        seen.append((min_frames.tolist(), max_min_frames, want_path))
        on = torch.tensor([[0, 2, 3]], dtype=torch.int32)
        return (on, on + torch.tensor([[2, 1, 2]], dtype=torch.int32), torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int32),
                torch.tensor([[1, 1, 3, 5, 5]], dtype=torch.int32))

    for name in dir(ops):
        if name.startswith(("viterbi_", "alignment_posteriors")):
            monkeypatch.setattr(ops, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("another entry was launched")))
    monkeypatch.setattr(ops, "viterbi_min_duration_batch", entry)
    em, lab = torch.zeros((1, 5, 4)), torch.tensor([[3, 5, 7]], dtype=torch.int32)
    n_lab, nf = torch.tensor([3], dtype=torch.int32), torch.tensor([5], dtype=torch.int32)
    mf = torch.tensor([[2, 1, 2]], dtype=torch.int32)
    r = ua.run_min_duration_lattice(em, lab, n_lab, nf, mf)
    assert seen == [([[2, 1, 2]], 2, True)]
    assert isinstance(r, ua.RepeatLatticeResult) and r.path.tolist() == [[1, 1, 3, 5, 5]] and r.occupancy is None
    skip = torch.full((1, 4), -1, dtype=torch.int32)
    win = (torch.zeros((1, 7), dtype=torch.int32), torch.full((1, 7), 5, dtype=torch.int32))
    rows = torch.full((1, 3), -1, dtype=torch.int32)
    for kw in (dict(skip_from=skip), dict(windows=win), dict(repeat_from=rows), dict(line_start=rows + 2)) + tuple(
            dict(confidence=c) for c in ("plain", "span", "anchored", "sheet", "repeat", "song", "lines")):
        with pytest.raises(ValueError, match="min_frames"):
            ua.run_min_duration_lattice(em, lab, n_lab, nf, mf, **kw)
    assert len(seen) == 1
    assert ua.MIN_DURATION_DP == "viterbi_min_duration_batch" and ua.MIN_DURATION_DP not in {r.dp for r in ua.ROUTES.values()} and len(ua.ROUTES) == 28

    # align_labels: the emissions are asked for with needed=True, the provider's own DP result is dropped, the segments come from the path
    asked = []

    def emissions_of(lab_x, n_x, needed=True):
        asked.append(needed)
        return ("the provider's plain DP",) * 4, em

    args = ("align", emissions_of, lab, n_lab, [[3, 5, 7]], [5], 5, None, 0.02, None, 2, None, None, 0.0, None, None, 0.0)
    out = ua.align_labels(*args, True, None, False, min_frames=mf)
    assert asked == [True] and len(seen) == 2
    assert out == ([[[0.0, 0.04], [0.04, 0.06], [0.06, 0.1]]], [[(0, 0.0, 0.04), (1, 0.04, 0.06), (2, 0.06, 0.1)]])
    assert ua.align_labels(*args, False, None, False, min_frames=mf) == out[0] and len(seen) == 3
    for kw in (dict(line_start=rows + 2), dict(off=object())):
        with pytest.raises(ValueError, match="min_duration"):
            ua.align_labels(*args, False, None, False, min_frames=mf, **kw)
    with pytest.raises(ValueError, match="min_duration"):
        ua.align_labels(*args[:9], "plain", *args[10:], False, None, False, min_frames=mf)
    with pytest.raises(ValueError, match="min_duration"):
        ua.align_labels(*args[:11], skip, *args[12:], False, None, False, min_frames=mf)
    assert len(seen) == 3 and asked == [True, True]


# ------------------------------------------------------------------------------------------------ 6. keyword positions and defaults
def test_keyword_positions_and_defaults():
    from lyricalignment_amd import ops
    from lyricalignment_amd.harness import align_record_lines, align_records
    from lyricalignment_amd.module.align_model import AlignModel
    from lyricalignment_amd.utils import alignment as ua
    for f in (ua.perform_viterbi, ua.perform_viterbi_ctc, ua._perform, AlignModel.align):
        names = list(inspect.signature(f).parameters)
        i = names.index("min_duration")                                    # between the readings and the line starts: nothing pinned moves
        assert names[i - 1: i + 3] == ["return_readings", "min_duration", "line_starts", "line_jump_penalty"], f.__name__
        assert names[-3:] == ["return_pronunciation", "pronunciation_classes", "pronunciation_top_k"], f.__name__
        assert inspect.signature(f).parameters["min_duration"].default is None
    names = list(inspect.signature(ua.align_labels).parameters)
    assert names[-2:] == ["min_frames", "pron"] and names[names.index("line_start"): names.index("line_start") + 3] == ["line_start", "line_jump_penalty", "off"]
    assert list(inspect.signature(ua.run_min_duration_lattice).parameters)[:5] == ["em", "lab", "n_lab", "nf", "min_frames"]
    assert list(inspect.signature(ua.run_lattice).parameters)[-2:] == ["line_start", "line_jump_penalty"]      # run_lattice keeps its list
    sig = inspect.signature(ops.viterbi_min_duration_batch).parameters
    assert list(sig) == ["em", "labels", "n_labels", "n_frames", "min_frames", "max_min_frames", "want_path"]
    assert sig["max_min_frames"].default is None and sig["want_path"].default is True
    assert "viterbi_min_duration" not in ops._ENTRIES and len(ops._ENTRIES) == 11                              # a wrapper of its own
    for f in (align_records, align_record_lines):
        sig = inspect.signature(f).parameters
        assert list(sig)[-1] == "min_duration" and sig["min_duration"].default is None
    for doc in (ua.perform_viterbi.__doc__, AlignModel.align.__doc__, ops.viterbi_min_duration_batch.__doc__):
        assert "min_duration" in doc or "min_frames" in doc
        assert "been tuned on real singing" in " ".join(doc.lower().split())


# ------------------------------------------------------------------------------------------------ 7. the library's host face
def test_the_entry_points_are_declared_exported_and_check_arguments_on_the_host():
    from lyricalignment_amd import _lib
    text = open(os.path.join(ROOT, "include", "lyricalign.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    C = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
    for name in ("la_viterbi_min_duration_workspace_bytes", "la_viterbi_min_duration_batch"):
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert decl, f"{name} not declared in lyricalign.h"
        assert name in _lib.SYMBOLS and _lib.SYMBOLS[name][0] is ctypes.c_int32
        args = [a.strip() for a in decl.group(1).split(",")]
        assert len(args) == len(_lib.SYMBOLS[name][1]), name
        for a, ctype in zip(args, _lib.SYMBOLS[name][1]):                # argument by argument
            if "*" in a:
                assert ctype in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)), (name, a)
            else:
                assert ctype is C[a.split()[-2]], (name, a)
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} not exported"
    arg_names = lambda fn: [a.strip().split()[-1].lstrip("*") for a in re.search(r"\bint\s+" + fn + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")]
    names, lines = arg_names("la_viterbi_min_duration_batch"), arg_names("la_viterbi_lines_batch")
    assert names == lines[:15] + ["min_frames", "min_frames_stride", "max_min_frames"] + lines[18:]
    assert lines[15:18] == ["line_start", "line_stride", "line_jump_penalty"]

    L = _lib.lib()
    need = ctypes.c_size_t(1)
    f = L.la_viterbi_min_duration_workspace_bytes
    # three 64-bit masks per (frame, R, wave), whatever the chain depth
    for shape, (r, nw) in (((32, 1500, 26), (1, 1)), ((2, 7000, 40), (1, 2)), ((3, 900, 238), (1, 8)), ((1, 600, 511), (1, 16)),
                           ((1, 600, 512), (2, 16)), ((1, 1200, 2500), (8, 16)), ((2, 50, 4095), (8, 16))):
        for depth in (1, 2, 3, 8):
            assert f(*shape, depth, ctypes.byref(need)) == _lib.LA_OK
            assert need.value == shape[0] * shape[1] * r * nw * 24, (shape, depth)
    assert f(1, 600, 4096, 8, ctypes.byref(need)) == _lib.LA_EUNSUPPORTED and "4095" in _lib.last_error()
    assert f(1, 600, 26, 8, None) == _lib.LA_EINVAL
    for depth in (0, 9, -1):
        assert f(1, 600, 26, depth, ctypes.byref(need)) == _lib.LA_EINVAL and "max_min_frames" in _lib.last_error()

    P = 16                                      # a non-null, aligned stand-in pointer: every call below is refused before any device call
    big = 1 << 40

    def call(em=P, labels=P, n_labels=P, n_frames=P, batch=2, T=100, Lmax=26, onset=P, offset=P, out_stride=26, score=P, status=P,
             min_frames=P, mf_stride=26, depth=8, path=P, path_stride=100, ws=P, ws_bytes=big, em_rs=27, labels_stride=26):
        return L.la_viterbi_min_duration_batch(em, T * em_rs, em_rs, labels, labels_stride, n_labels, n_frames, batch, T, Lmax, onset, offset,
                                               out_stride, score, status, min_frames, mf_stride, depth, path, path_stride, ws, ws_bytes, 0)

    for null in ("em", "labels", "n_labels", "n_frames", "onset", "offset", "score", "status", "min_frames"):
        assert call(**{null: 0}) == _lib.LA_EINVAL, null
        assert "null" in _lib.last_error() and "viterbi_min_duration_batch" in _lib.last_error()
    for depth in (0, 9, -2):
        assert call(depth=depth) == _lib.LA_EINVAL and "max_min_frames" in _lib.last_error() and "viterbi_min_duration_batch" in _lib.last_error()
    assert call(mf_stride=25) == _lib.LA_EINVAL and "strides" in _lib.last_error()
    assert call(out_stride=25) == _lib.LA_EINVAL and call(em_rs=26) == _lib.LA_EINVAL and call(labels_stride=25) == _lib.LA_EINVAL
    assert call(path_stride=99) == _lib.LA_EINVAL and "path_stride" in _lib.last_error()
    assert call(T=0) == _lib.LA_EINVAL and call(batch=-1) == _lib.LA_EINVAL
    assert call(Lmax=4096, out_stride=4096, em_rs=4097, labels_stride=4096, mf_stride=4096) == _lib.LA_EUNSUPPORTED
    assert "4095" in _lib.last_error()
    assert call(ws_bytes=2 * 100 * 24 - 1) == _lib.LA_EINVAL and "workspace too small" in _lib.last_error()
    assert call(ws=0) == _lib.LA_EINVAL
    assert call(ws=P + 4) == _lib.LA_EINVAL and "aligned" in _lib.last_error()
    assert call(batch=0) == _lib.LA_OK          # nothing to do, nothing enqueued


# ------------------------------------------------------------------------------------------------ 8. the harness
def test_the_harness_passes_min_duration_on_and_refuses_it_with_the_other_sheet_keywords():
    from types import SimpleNamespace
    from lyricalignment_amd.harness import PinyinClassLUT, align_record_lines, align_records
    seen = []

    class Model:
        def align(self, audios, labels, **kw):
            seen.append(kw)
            return [[[0.1 * i, 0.1 * i + 0.06] for i in range(len(labels[b]))] for b in range(len(audios))]

    lut = PinyinClassLUT(list("abcdefgh"), {c: i + 1 for i, c in enumerate("abcdefgh")})
    tok = lambda text: ["abcdefgh".index(c) for c in text]
    recs = [SimpleNamespace(audio=np.zeros(1600, np.float32), text="abc"), SimpleNamespace(audio=np.zeros(3200, np.float32), text="de")]
    out = align_records(Model(), recs, lut, tok, min_duration=0.06)
    assert [kw.get("min_duration") for kw in seen] == [0.06, 0.06] and [len(o) for o in out] == [3, 2]
    seen.clear()
    align_records(Model(), recs, lut, tok)
    assert all("min_duration" not in kw for kw in seen)                          # None: the call as it was
    seen.clear()
    align_records(Model(), recs, lut, tok, batch_size=2, min_duration=0.06)
    assert [kw.get("min_duration") for kw in seen] == [0.06] and seen[0]["per_clip"] is True
    with pytest.raises(ValueError, match="min_duration.*with_confidence"):
        align_records(Model(), recs, lut, tok, with_confidence=True, min_duration=0.06)
    seen.clear()
    lines = ["ab", "cde"]
    out = align_record_lines(Model(), np.zeros(1600, np.float32), lines, [False, False], lut, tok, min_duration=0.06)
    assert seen[0]["min_duration"] == 0.06 and [len(o) for o in out] == [2, 3]
    for kw in (dict(with_confidence=True), dict(repeatable=[False, True]), dict(off_sheet=True)):
        with pytest.raises(ValueError, match=rf"min_duration.*{list(kw)[0]}"):
            align_record_lines(Model(), np.zeros(1600, np.float32), lines, [False, False], lut, tok, min_duration=0.06, **kw)
    with pytest.raises(ValueError, match="min_duration.*optional"):
        align_record_lines(Model(), np.zeros(1600, np.float32), lines, [False, True], lut, tok, min_duration=0.06)
    assert len(seen) == 1
