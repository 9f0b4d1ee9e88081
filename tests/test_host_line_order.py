"""CPU-only checks of the alignment DP with free line order: the all-pairs float64 yardstick (tests/line_order_reference.py) against
exhaustive path enumeration, the planted performance the feature exists for, its two identities (penalty +inf = the plain lattice, one
line = the repeat lattice with the whole sheet repeatable), the host helpers, every refusal of the Python surface with the device
stubbed, keyword positions, the host face of la_viterbi_lines_batch (declared, exported, argument checks answered before any device
call) and harness.align_free_order on a stubbed align."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import line_order_reference as lo
import optional_spans_reference as osr
import repeat_spans_reference as rr
from conftest import ROOT


# ------------------------------------------------------------------------------------------------ 1. exhaustive enumeration
def test_the_restatement_equals_exhaustive_enumeration():
    """Random lattices of 3 labels x 6 frames with 1, 2 and 3 lines, equal and unequal neighbour classes, penalties 0 / 0.3 / 2: the DP's
    score is the maximum over ALL lattice paths (free starts and ends included), accumulated in the same order."""
    rs = np.random.RandomState(0)
    seen_lines, seen_pen, n_jump, n_equal = set(), set(), 0, 0
    for case in range(90):
        L, T = 3, 6
        labels = [int(v) for v in rs.randint(1, 3, size=L)]                        # two classes: equal neighbours are common
        n_lines = 1 + case % 3
        starts = [0] + sorted(rs.choice(np.arange(1, L), size=n_lines - 1, replace=False).tolist())
        ls = [1 if n in starts else 0 for n in range(L)]
        pen = (0.0, 0.3, 2.0)[(case // 3) % 3]
        em = np.log(rs.dirichlet(np.ones(L + 1), size=T)).astype(np.float32)
        got = lo.viterbi(em, labels, ls, pen)
        want = lo.enumerate_best(em, labels, ls, pen)
        assert got[3] == lo.LA_OK and want is not None
        assert got[2] == want, (case, labels, ls, pen, got[2], want)
        seen_lines.add(n_lines), seen_pen.add(pen)
        n_jump += got.n_jumps > 0 or got.free_start or got.free_end
        n_equal += any(labels[a] == labels[e - 1] for a in starts for e in starts[1:] + [L])
    assert seen_lines == {1, 2, 3} and seen_pen == {0.0, 0.3, 2.0} and n_jump > 20 and n_equal > 20, (n_jump, n_equal)


# ------------------------------------------------------------------------------------------------ 2. the planted performance
def test_a_sheet_sung_in_another_order_is_recovered():
    """4 lines x 6 labels sung as lines 2, 0, 1, 1, 2, three frames per label: the order is found, line 3 is unsung, the path starts in
    line 2 and does not end in the last line."""
    c = lo.planted(1, 5 * (18 + 2), [6] * 4, [2, 0, 1, 1, 2], 3, 2)
    r = lo.viterbi(c["em"], c["lab"], c["ls"], 1.0)
    assert r[3] == lo.LA_OK
    assert lo.line_order(r[4], c["ls"], 24) == [2, 0, 1, 1, 2]
    assert all(v == -1 for v in r[0][18:]) and all(v == -1 for v in r[1][18:]) and all(v >= 0 for v in r[0][:18])
    assert r[4][0] == 2 * 12 + 1 and r.free_start
    assert r[4][-1] in (2 * 18 - 1, 2 * 18) and r.free_end
    assert r.n_jumps == 2                                                              # 2 -> 0 and 1 -> 1; 0 -> 1 and 1 -> 2 are the sheet's own arcs
    visits = lo.segments(r[4])
    assert [n for n, _, _ in visits] == [n for m in (2, 0, 1, 1, 2) for n in range(6 * m, 6 * m + 6)]
    assert r[0][12] == 0 and r[0][6] == visits[12][1]                                 # the FIRST visit
    # a prohibitive penalty: the plain lattice's path, no jump anywhere
    mono = lo.viterbi(c["em"], c["lab"], c["ls"], float("inf"))
    assert mono.n_jumps == 0 and not mono.free_start and not mono.free_end and mono[2] < r[2]


# ------------------------------------------------------------------------------------------------ 3. the two identities
def test_an_infinite_penalty_is_the_plain_lattice_and_one_line_is_the_repeat_lattice():
    rs = np.random.RandomState(4)
    for case in range(40):
        L, T = int(rs.randint(2, 10)), int(rs.randint(24, 60))
        labels = [int(v) for v in rs.randint(1, 4, size=L)]
        em = np.log(rs.dirichlet(np.ones(L + 1), size=T)).astype(np.float32)
        starts = [0] + sorted(rs.choice(np.arange(1, L), size=int(rs.randint(0, L)), replace=False).tolist())
        ls = [1 if n in starts else 0 for n in range(L)]
        got = lo.viterbi(em, labels, ls, float("inf"))
        want = osr.viterbi_spans(em, labels, [-1] * (L + 1), 0.0)
        assert want[3] == lo.LA_OK and tuple(got) == tuple(want), case
        # one line: the whole sheet repeatable, the same penalty
        pen = (0.0, 0.3, 2.0)[case % 3]
        one = lo.viterbi(em, labels, [1] + [0] * (L - 1), pen)
        want = rr.viterbi(em, labels, None, 0.0, [L] + [-1] * (L - 1), pen, rows=True)
        assert tuple(one) == tuple(want), (case, pen)
        assert one.n_jumps == want.n_repeats


def test_results_for_empty_and_invalid_clips():
    em = np.zeros((4, 3), dtype=np.float32)
    assert tuple(lo.viterbi(em, [], [], 0.0)) == ([], [], 0.0, lo.LA_EEMPTY, [])
    assert tuple(lo.viterbi(em, [1, 2], [0, 1], 0.0)) == ([-1, -1], [-1, -1], 0.0, lo.LA_EINVAL, [])


# ------------------------------------------------------------------------------------------------ 4. host helpers, validation, refusals
def test_lines_from_lengths_and_row_validation():
    from lyricalignment_amd.utils.alignment import _line_start_of, lines_from_lengths
    assert lines_from_lengths([2, 3, 1]) == [1, 0, 1, 0, 0, 1]
    assert lines_from_lengths([4]) == [1, 0, 0, 0]
    for bad in ([], [2, 0], [-1]):
        with pytest.raises(ValueError):
            lines_from_lengths(bad)
    lists = [[1, 2, 3, 4], [5, 6], []]
    assert _line_start_of("f", None, lists) is None
    rows = _line_start_of("f", [[0, 2], [0], []], lists)
    assert rows.tolist() == [[1, 0, 1, 0], [1, 0, 0, 0], [0, 0, 0, 0]] and str(rows.dtype) == "torch.int32"
    assert _line_start_of("f", [[0, 1, 2, 3], [0, 1], None], lists).tolist() == [[1, 1, 1, 1], [1, 1, 0, 0], [0, 0, 0, 0]]
    for bad in ([[1, 2], [0], []], [[0, 2, 2], [0], []], [[0, 3, 2], [0], []], [[0, 4], [0], []], [[0], [0, 2], []], [[], [0], []],
                [[0], [0], [0]], [[0, 1.5], [0], []], [[0, True], [0], []], [[0], [0]]):
        with pytest.raises(ValueError, match="line_starts"):
            _line_start_of("f", bad, lists)
    with pytest.raises(NotImplementedError, match="4095"):
        _line_start_of("f", [[0]], [list(range(4096))])
    assert _line_start_of("f", [[0, 4094]], [list(range(4095))].copy()).shape == (1, 4095)


class _Stop(Exception):
    pass


REFUSED = dict(optional_spans=[[(0, 1)]], repeat_spans=[[(0, 2)]], onset_anchors=[[(0, 0.1, 0.1)]], char_windows=[[(0, 0.0, 0.2)]],
               off_sheet=[[1]])
CONFIDENCES = ("return_confidence", "return_span_confidence", "return_anchored_confidence", "return_sheet_confidence",
               "return_repeat_confidence", "return_song_confidence")


def test_bad_rows_and_every_refusal_come_before_a_device_is_asked_for(monkeypatch):
    from lyricalignment_amd import ops
    from lyricalignment_amd.module.align_model import AlignModel
    from lyricalignment_amd.utils import alignment as ua
    logits = torch.zeros((1, 20, 12))
    labels = torch.tensor([[3, 5, 7]])

    def launch(*a, **k):
        raise _Stop()

    monkeypatch.setattr(ua, "_device_of", launch)
    monkeypatch.setattr(ops, "emissions_from_logits", launch)
    monkeypatch.setattr(ops, "viterbi_lines_batch", launch)

    class Unbuilt(AlignModel):                                          # align's keyword checks come before the engine exists
        def __init__(self):
            pass

        def engine(self):
            raise _Stop()

    audio = [np.zeros(16000, np.float32)]
    calls = [lambda **kw: f(logits, labels, **kw) for f in (ua.perform_viterbi, ua.perform_viterbi_ctc)]
    calls.append(lambda **kw: AlignModel.align(Unbuilt(), audio, labels, **kw))
    for n, call in enumerate(calls):
        for bad in ([[1]], [[0, 0]], [[0, 2, 1]], [[0, 3]], [[]], [[0], [0]]):
            with pytest.raises(ValueError, match="line_starts"):
                call(line_starts=bad)
        for name, value in REFUSED.items():
            with pytest.raises(ValueError, match=rf"line_starts.*{name}"):
                call(line_starts=[[0, 2]], **{name: value})
        for pen in (-1.0, float("nan")):
            with pytest.raises(ValueError, match="line_jump_penalty"):
                call(line_starts=[[0, 2]], line_jump_penalty=pen)
        with pytest.raises(NotImplementedError, match="4095"):
            (ua.perform_viterbi if n < 2 else lambda *a, **k: AlignModel.align(Unbuilt(), audio, *a[1:], **k))(
                torch.zeros((1, 4, 12)), [list(np.arange(4096) % 11 + 1)], line_starts=[[0]])
        with pytest.raises(_Stop):                                      # good keywords are accepted (and go on to the device)
            call(line_starts=[[0, 2]], line_jump_penalty=0.5, return_segments=True)
        with pytest.raises(_Stop):                                      # all-empty companions are "not given"
            call(line_starts=[[0, 2]], optional_spans=[[]], off_sheet=[[]])
    for name in CONFIDENCES:
        with pytest.raises(ValueError, match=rf"line_starts.*{name}"):
            AlignModel.align(Unbuilt(), audio, labels, line_starts=[[0, 2]], **{name: True})
    # the _scored functions and the training entries do not have the keyword
    for name in dir(ua):
        if name.endswith("_scored") or name in ("anchored_alignment_loss", "anchored_loss_inputs"):
            assert "line_starts" not in inspect.signature(getattr(ua, name)).parameters, name


def test_run_lattice_routes_a_line_start_to_the_new_entry_and_refuses_the_rest(monkeypatch):
    from lyricalignment_amd import ops
    from lyricalignment_amd.utils import alignment as ua
    seen = []

    def entry(em, lab, n_lab, nf, line_start, line_jump_penalty=0.0):
        seen.append((line_start.tolist(), line_jump_penalty))
        z = torch.zeros((1, 3), dtype=torch.int32)
        return z, z + 1, torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int32), torch.ones((1, 5), dtype=torch.int32)

    for name in dir(ops):
        if name.startswith(("viterbi_", "alignment_posteriors")):
            monkeypatch.setattr(ops, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("another entry was launched")))
    monkeypatch.setattr(ops, "viterbi_lines_batch", entry)
    em, lab = torch.zeros((1, 5, 4)), torch.tensor([[3, 5, 7]], dtype=torch.int32)
    n_lab, nf = torch.tensor([3], dtype=torch.int32), torch.tensor([5], dtype=torch.int32)
    ls = torch.tensor([[1, 0, 1]], dtype=torch.int32)
    r = ua.run_lattice(em, lab, n_lab, nf, line_start=ls, line_jump_penalty=0.75)
    assert seen == [([[1, 0, 1]], 0.75)]
    assert isinstance(r, ua.RepeatLatticeResult) and r.path.tolist() == [[1] * 5] and r.occupancy is None
    skip = torch.full((1, 4), -1, dtype=torch.int32)
    win = (torch.zeros((1, 7), dtype=torch.int32), torch.full((1, 7), 5, dtype=torch.int32))
    rf = torch.full((1, 3), -1, dtype=torch.int32)
    for kw in (dict(skip_from=skip), dict(windows=win), dict(repeat_from=rf)) + tuple(dict(confidence=c) for c in
                                                                                     ("plain", "span", "anchored", "sheet", "repeat", "song")):
        with pytest.raises(ValueError, match="line_start"):
            ua.run_lattice(em, lab, n_lab, nf, line_start=ls, **kw)
    assert len(seen) == 1
    assert ua.LINES_DP == "viterbi_lines_batch" and ua.LINES_DP not in {r.dp for r in ua.ROUTES.values()} and len(ua.ROUTES) == 28


# ------------------------------------------------------------------------------------------------ 5. keyword positions and defaults
def test_keyword_positions_and_defaults():
    from lyricalignment_amd import ops
    from lyricalignment_amd.harness import align_free_order, align_record_lines, align_record_lrc, align_song
    from lyricalignment_amd.module.align_model import AlignModel
    from lyricalignment_amd.utils import alignment as ua
    for f in (ua.perform_viterbi, ua.perform_viterbi_ctc, ua._perform, AlignModel.align):
        names = list(inspect.signature(f).parameters)
        assert names[-3:] == ["return_pronunciation", "pronunciation_classes", "pronunciation_top_k"], f.__name__
        i = names.index("line_starts")
        assert names[i: i + 3] == ["line_starts", "line_jump_penalty", "off_sheet"], f.__name__              # in front of off_sheet
        sig = inspect.signature(f).parameters
        assert sig["line_starts"].default is None and sig["line_jump_penalty"].default == 0.0
    names = list(inspect.signature(ua.align_labels).parameters)
    assert names[-1] == "pron" and names[names.index("line_start"): names.index("line_start") + 3] == ["line_start", "line_jump_penalty", "off"]
    names = list(inspect.signature(ua.run_lattice).parameters)
    assert names[-2:] == ["line_start", "line_jump_penalty"] and names[:12] == [
        "em", "lab", "n_lab", "nf", "skip_from", "windows", "skip_penalty", "confidence", "boundary_window", "dp", "repeat_from", "repeat_penalty"]
    assert list(inspect.signature(ops.viterbi_lines_batch).parameters) == ["em", "labels", "n_labels", "n_frames", "line_start", "line_jump_penalty"]
    assert inspect.signature(ops.viterbi_lines_batch).parameters["line_jump_penalty"].default == 0.0
    assert "viterbi_lines" not in ops._ENTRIES and len(ops._ENTRIES) == 11                          # a wrapper of its own
    assert list(inspect.signature(align_free_order).parameters) == ["model", "audio", "lines", "lut", "tokenize", "use_ctc_loss", "line_jump_penalty",
                                                                   "heteronyms"]
    sig = inspect.signature(align_free_order).parameters
    assert sig["use_ctc_loss"].default is True and sig["line_jump_penalty"].default == 0.0 and sig["heteronyms"].default is None
    for f in (align_record_lines, align_record_lrc, align_song):                                    # the sheet functions keep their signatures
        assert "line_starts" not in inspect.signature(f).parameters and "line_jump_penalty" not in inspect.signature(f).parameters
    for doc in (ua.perform_viterbi.__doc__, AlignModel.align.__doc__, align_free_order.__doc__, ops.viterbi_lines_batch.__doc__):
        assert "line_jump_penalty" in doc and "not been tuned on real singing" in " ".join(doc.lower().split())


# ------------------------------------------------------------------------------------------------ 6. the library's host face
def test_the_entry_points_are_declared_exported_and_check_arguments_on_the_host():
    from lyricalignment_amd import _lib
    text = open(os.path.join(ROOT, "include", "lyricalign.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    C = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
    for name in ("la_viterbi_lines_workspace_bytes", "la_viterbi_lines_batch"):
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
    names = [a.strip().split()[-1].lstrip("*") for a in re.search(r"\bint\s+la_viterbi_lines_batch\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")]
    plain = [a.strip().split()[-1].lstrip("*") for a in re.search(r"\bint\s+la_viterbi_batch\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")]
    assert names == plain[:15] + ["line_start", "line_stride", "line_jump_penalty", "path", "path_stride"] + plain[15:]

    L = _lib.lib()
    need = ctypes.c_size_t(1)
    f = L.la_viterbi_lines_workspace_bytes
    # two 64-bit masks per (frame, R, wave) and two int32 per frame
    for shape, (r, nw) in (((32, 1500, 26), (1, 1)), ((2, 7000, 40), (1, 2)), ((3, 900, 238), (1, 8)), ((1, 600, 511), (1, 16)),
                           ((1, 600, 512), (2, 16)), ((1, 1200, 2500), (8, 16)), ((2, 50, 4095), (8, 16))):
        assert f(*shape, ctypes.byref(need)) == _lib.LA_OK
        assert need.value == shape[0] * shape[1] * (r * nw * 16 + 8), shape
    assert f(1, 600, 4096, ctypes.byref(need)) == _lib.LA_EUNSUPPORTED and "4095" in _lib.last_error()
    assert f(1, 600, 26, None) == _lib.LA_EINVAL

    P = 16                                      # a non-null, aligned stand-in pointer: every call below is refused before any device call
    big = 1 << 40

    def call(em=P, labels=P, n_labels=P, n_frames=P, batch=2, T=100, Lmax=26, onset=P, offset=P, out_stride=26, score=P, status=P,
             line_start=P, line_stride=26, penalty=0.0, path=P, path_stride=100, ws=P, ws_bytes=big, em_rs=27, labels_stride=26):
        return L.la_viterbi_lines_batch(em, T * em_rs, em_rs, labels, labels_stride, n_labels, n_frames, batch, T, Lmax, onset, offset,
                                        out_stride, score, status, line_start, line_stride, penalty, path, path_stride, ws, ws_bytes, 0)

    for null in ("em", "labels", "n_labels", "n_frames", "onset", "offset", "score", "status", "line_start"):
        assert call(**{null: 0}) == _lib.LA_EINVAL, null
        assert "null" in _lib.last_error() and "viterbi_lines_batch" in _lib.last_error()
    for pen in (-0.5, float("nan"), float("-inf")):
        assert call(penalty=pen) == _lib.LA_EINVAL and "line_jump_penalty" in _lib.last_error()
    assert call(line_stride=25) == _lib.LA_EINVAL and "strides" in _lib.last_error()
    assert call(out_stride=25) == _lib.LA_EINVAL and call(em_rs=26) == _lib.LA_EINVAL and call(labels_stride=25) == _lib.LA_EINVAL
    assert call(path_stride=99) == _lib.LA_EINVAL and "path_stride" in _lib.last_error()
    assert call(T=0) == _lib.LA_EINVAL and call(batch=-1) == _lib.LA_EINVAL
    assert call(Lmax=4096, out_stride=4096, em_rs=4097, labels_stride=4096, line_stride=4096) == _lib.LA_EUNSUPPORTED
    assert "4095" in _lib.last_error()
    assert call(ws_bytes=2 * 100 * 24 - 1) == _lib.LA_EINVAL and "workspace too small" in _lib.last_error()
    assert call(ws=0) == _lib.LA_EINVAL
    assert call(ws=P + 4) == _lib.LA_EINVAL and "aligned" in _lib.last_error()
    assert call(batch=0) == _lib.LA_OK          # nothing to do, nothing enqueued


# ------------------------------------------------------------------------------------------------ 7. the harness
def test_align_free_order_from_a_stubbed_align():
    from lyricalignment_amd.harness import PinyinClassLUT, align_free_order
    lines = ["ab", "cde", "f", "gh"]
    seen = {}

    class Model:
        def align(self, audios, labels, **kw):
            seen.update(kw, labels=labels.tolist(), n_audio=len(audios))
            # sung: line 1, line 0, line 1, line 2, line 1 (line 3 never)
            sung = [2, 3, 4, 0, 1, 2, 3, 4, 5, 2, 3, 4]
            segments = [[(n, 0.1 * i, 0.1 * i + 0.05) for i, n in enumerate(sung)]]
            seconds = [[[0.3, 0.35], [0.4, 0.45], [0.0, 0.05], [0.1, 0.15], [0.2, 0.25], [0.8, 0.85], None, None]]
            return seconds, segments

    lut = PinyinClassLUT(["a", "b", "c", "d", "e", "f", "g", "h"], {c: i + 1 for i, c in enumerate("abcdefgh")})
    out = align_free_order(Model(), np.zeros(1600, np.float32), lines, lut, lambda line: ["abcdefgh".index(c) for c in line], line_jump_penalty=0.5)
    assert seen["line_starts"] == [[0, 2, 5, 6]] and seen["line_jump_penalty"] == 0.5 and seen["return_segments"] is True
    assert seen["use_ctc"] is True and seen["n_audio"] == 1 and len(seen["labels"][0]) == 8
    assert not any(k in seen for k in ("optional_spans", "repeat_spans", "off_sheet"))
    assert set(out) == {"occurrences", "order", "unsung"}
    assert out["order"] == [1, 0, 1, 2, 1] and out["unsung"] == [3]
    occ = out["occurrences"]
    assert [len(o) for o in occ] == [1, 3, 1, 0]
    assert [c for _, _, c in occ[1][2]] == ["c", "d", "e"] and occ[1][2][0][:2] == [pytest.approx(0.9), pytest.approx(0.95)]
    assert occ[0] == [[[pytest.approx(0.3), pytest.approx(0.35), "a"], [pytest.approx(0.4), pytest.approx(0.45), "b"]]]
    with pytest.raises(ValueError, match="align_free_order"):
        align_free_order(Model(), np.zeros(1600, np.float32), lines, lut, lambda line: [0])
