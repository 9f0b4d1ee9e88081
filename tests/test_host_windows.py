"""CPU-only checks of anchored alignment (per-state frame windows in the alignment DP): the float64 yardstick
(tests/windows_reference.py) against tests/optional_spans_reference.py and oracle/viterbi_python.py with open windows and against
exhaustive enumeration of the paths inside the windows, the host helpers (windows_from_anchors, parse_lrc), the planted repeated phrase
the feature exists for, and the host face of la_viterbi_windows_batch (declared, exported, argument checks answered before any device
call)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import optional_spans_reference as osr
import windows_reference as wr
from conftest import ROOT, e2e_cases

HOP = 0.02


def _random_spans(rs, L, p=0.5):
    sf = [-1] * (L + 1)
    for n in range(1, L + 1):
        if rs.rand() < p:
            sf[n] = int(rs.randint(0, n))
    return sf


def _em64(rs, T, labels):
    """Compact emissions [T, L+1] in multiples of 1/64 from -4 to 0 (exact in float32 and in every float64 sum of the DP); equal labels
    carry identical columns."""
    V = max(labels)
    lp = -rs.randint(0, 257, size=(T, V)) / 64.0
    ls = -rs.randint(0, 257, size=(T, 1)) / 64.0
    return np.concatenate([ls, lp[:, np.asarray(labels) - 1]], axis=1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. open windows = the lattices of today
def test_open_windows_equal_the_span_reference_and_the_oracle_on_the_golden_cases():
    """Every golden viterbi_e2e case with every window [0, T): onset, offset, score, status and path of viterbi_spans, without spans and
    with random ones (penalty 0.5); without spans dp and bt also equal oracle.viterbi_python.viterbi_lattice's cell by cell."""
    from oracle.viterbi_python import viterbi_lattice
    rs = np.random.RandomState(11)
    n = 0
    for _, _, em, label, _ in e2e_cases():
        labels = [int(v) for v in label]
        T, L = em.shape[0], len(labels)
        lo, hi = wr.open_windows(L, T)
        assert wr.viterbi_windows(em, labels, lo, hi) == osr.viterbi_spans(em, labels, [-1] * (L + 1))
        sf = _random_spans(rs, L, 0.3)
        assert wr.viterbi_windows(em, labels, lo, hi, sf, 0.5) == osr.viterbi_spans(em, labels, sf, 0.5)
        dense = {v: i + 1 for i, v in enumerate(sorted(set(labels)))}
        lab = np.asarray([dense[v] for v in labels])
        lp = np.zeros((T, len(dense)), np.float32)
        lp[:, lab - 1] = em[:, 1: L + 1]
        dp_o, bt_o = viterbi_lattice(lp, em[:, :1], lab)
        dp, bt, jumped = wr.lattice(em, labels, lo, hi)
        assert np.array_equal(np.asarray(dp), dp_o) and np.array_equal(np.asarray(bt)[1:], bt_o[1:])
        assert not np.asarray(jumped).any()
        # the row-at-a-time form of the restatement fills the same cells, under narrowed windows and with spans too
        lo2 = [int(rs.randint(0, T // 2 + 1)) if rs.rand() < 0.3 else 0 for _ in range(2 * L + 1)]
        hi2 = [int(rs.randint(T // 2, T + 1)) if rs.rand() < 0.3 else T for _ in range(2 * L + 1)]
        for a, b in zip(wr.lattice(em, labels, lo2, hi2, sf, 0.5), wr.lattice_rows(em, labels, lo2, hi2, sf, 0.5)):
            assert np.array_equal(np.asarray(a)[1:], b[1:]) and np.array_equal(np.asarray(a[0], dtype=b.dtype)[: 2], b[0][: 2])
        n += 1
    assert n >= 10


# ------------------------------------------------------------------------------------------------ 2. exhaustive enumeration
def test_score_equals_enumeration_of_the_paths_inside_the_windows():
    """1500 random cases, T <= 7, L <= 3, emissions in multiples of 1/64, half of them with spans, penalties 0 / 0.5 / 1, about a third
    of the states with a random lo and a third with a random hi: the score == the best over all lattice paths inside the windows (to the
    bit), the reported path lies inside its windows and is a path of the lattice; where no path exists the status is LA_EINFEASIBLE."""
    rs = np.random.RandomState(0)
    none, with_spans_ok, dead = 0, 0, 0
    for case in range(1500):
        T, L = int(rs.randint(1, 8)), int(rs.randint(1, 4))
        labels = [int(v) for v in rs.randint(1, 4, size=L)]
        sf = _random_spans(rs, L) if case % 2 else [-1] * (L + 1)
        pen = (0.0, 0.5, 1.0)[case % 3]
        em = _em64(rs, T, labels)
        S = 2 * L + 1
        lo = [int(rs.randint(0, T + 1)) if rs.rand() < 0.3 else 0 for _ in range(S)]
        hi = [int(rs.randint(0, T + 1)) if rs.rand() < 0.3 else T for _ in range(S)]
        want = wr.enumerate_best(em, labels, lo, hi, sf, pen)
        on, off, score, status, path = wr.viterbi_windows(em, labels, lo, hi, sf, pen)
        if want is None:
            none += 1
            assert status == wr.LA_EINFEASIBLE, (case, T, labels, sf, lo, hi)
            if score == wr.NINF:
                dead += 1
                assert on == [-1] * L and off == [-1] * L and path == []
            continue
        assert score == want and status == wr.LA_OK, (case, T, labels, sf, pen, lo, hi, score, want)
        assert wr.viterbi_windows(em, labels, lo, hi, sf, pen, rows=True) == (on, off, score, status, path)
        assert all(lo[s] <= t < hi[s] for t, s in enumerate(path)), (case, path, lo, hi)
        preds = osr.arcs(labels, sf)
        assert path[0] in (0, 1) and path[-1] in (S - 1, S - 2)
        for t in range(1, T):
            assert path[t - 1] in [src for src, _ in preds[path[t]]]
        with_spans_ok += case % 2
    print(f"{none} of 1500 cases without a path ({dead} with a final score of -inf), {with_spans_ok} feasible cases with spans")
    assert 300 < none < 1200 and dead > 100 and with_spans_ok > 100


# ------------------------------------------------------------------------------------------------ 3. windows_from_anchors
def test_windows_from_anchors_forms_rounding_and_errors():
    from lyricalignment_amd.utils.alignment import windows_from_anchors as wfa
    assert wfa(3, 50) == ([0] * 7, [50] * 7)
    assert wfa(0, 9) == ([0], [9])
    # a character's window: lo = ceil(lo_s / hop), hi = floor(hi_s / hop) with the 1e-9 guard against the division's rounding
    lo, hi = wfa(3, 50, char_windows=[(1, 0.10, 0.30)])
    assert lo == [0, 0, 0, 5, 0, 0, 0] and hi == [50, 50, 50, 15, 50, 50, 50]
    assert 0.7 / 0.1 < 7.0 and 0.14 / 0.02 > 7.0                                              # (float64: 6.999999999999999, 7.000000000000001)
    assert wfa(1, 50, char_windows=[(0, 0.3, 0.7)], hop_size_second=0.1) == ([0, 3, 0], [50, 7, 50])
    assert wfa(1, 50, char_windows=[(0, 0.14, None)]) == ([0, 7, 0], [50, 50, 50])
    lo, hi = wfa(3, 50, char_windows=[(1, 0.101, 0.299)])
    assert (lo[3], hi[3]) == (6, 14)
    lo, hi = wfa(3, 50, char_windows=[(0, None, 0.2), (2, 0.5, None)])
    assert lo == [0, 0, 0, 0, 0, 25, 0] and hi == [50, 10, 50, 50, 50, 50, 50]
    lo, hi = wfa(3, 50, char_windows=[(1, 0.1, 0.6), (1, 0.2, None), (1, None, 0.4)])          # constraints on one state intersect
    assert (lo[3], hi[3]) == (10, 20)
    lo, hi = wfa(3, 50, char_windows=[(1, -5.0, 1e9)])                                        # beyond the clip: open
    assert (lo[3], hi[3]) == (0, 50)
    # an onset anchor on a frame: frames 8..12 lie within 0.04 s of 0.2 s; the character may not start before 8, and every state before
    # it has ended by 12
    lo, hi = wfa(3, 50, onset_anchors=[(2, 0.2, 0.04)])
    assert lo == [0, 0, 0, 0, 0, 8, 0] and hi == [12, 12, 12, 12, 12, 50, 50]
    lo, hi = wfa(3, 50, onset_anchors=[(2, 0.21, 0.02)])                                      # between frames: 9.5 .. 11.5 -> 10 .. 11
    assert lo[5] == 10 and hi[:5] == [11] * 5
    lo, hi = wfa(3, 50, onset_anchors=[(2, 0.2, 0.0)])                                        # tol 0 on a frame: that frame
    assert lo[5] == 10 and hi[:5] == [10] * 5
    lo, hi = wfa(3, 50, onset_anchors=[(2, 0.212, 0.0)])                                      # tol 0 between frames: the nearest frame
    assert lo[5] == 11 and hi[:5] == [11] * 5
    lo, hi = wfa(3, 50, onset_anchors=[(2, 0.205, 0.0)])
    assert lo[5] == 10 and hi[:5] == [10] * 5
    lo, hi = wfa(3, 50, onset_anchors=[(0, 0.0, 0.0)])                                        # the first character starts at frame 0
    assert lo == [0] * 7 and hi == [0] + [50] * 6
    # both forms and two anchors: everything intersects
    lo, hi = wfa(3, 50, char_windows=[(0, 0.04, 0.5), (2, 0.3, None)], onset_anchors=[(1, 0.4, 0.1), (2, 0.6, 0.1)])
    assert lo == [0, 2, 0, 15, 0, 25, 0] and hi == [25, 25, 25, 35, 35, 50, 50]
    lo, hi = wfa(2, 100, onset_anchors=[(1, 1.0, 0.5)], hop_size_second=0.1)
    assert lo == [0, 0, 0, 5, 0] and hi == [15, 15, 15, 100, 100]
    for bad in (dict(char_windows=[(3, 0.0, 1.0)]), dict(char_windows=[(-1, 0.0, 1.0)]), dict(onset_anchors=[(3, 0.1, 0.1)]),
                dict(onset_anchors=[(-1, 0.1, 0.1)]), dict(onset_anchors=[(1, 0.1, -0.01)]), dict(onset_anchors=[(1, float("nan"), 0.1)]),
                dict(onset_anchors=[(1, 0.1, float("nan"))]), dict(char_windows=[(1, float("nan"), None)]),
                dict(char_windows=[(1, None, float("nan"))]), dict(char_windows=[(float("nan"), 0.0, 1.0)])):
        with pytest.raises(ValueError):
            wfa(3, 50, **bad)


def test_anchors_and_windows_around_a_known_path_hold_in_the_result():
    """300 random clips (T 20..60, L 1..6, half with spans): anchors and character windows are laid around the unconstrained path, off
    the truth by up to the tolerance, so the case is feasible by construction.  Every case must come back LA_OK, every reported onset of an
    anchored character inside the anchor's frame range, every windowed character's segment inside its window."""
    from lyricalignment_amd.utils.alignment import windows_from_anchors as wfa
    rs = np.random.RandomState(5)
    n_moved = 0
    for case in range(300):
        T, L = int(rs.randint(20, 61)), int(rs.randint(1, 7))
        labels = [int(v) for v in rs.randint(1, 5, size=L)]
        sf = _random_spans(rs, L, 0.3) if case % 2 else [-1] * (L + 1)
        em = _em64(rs, T, labels)
        on0, off0, _, st0, _ = osr.viterbi_spans(em, labels, sf, 0.5)
        assert st0 == osr.LA_OK
        sung = [n for n in range(L) if on0[n] >= 0]
        anchors, ranges = [], {}
        for n in rs.permutation(sung)[: int(rs.randint(1, 4))]:
            tol = float(rs.randint(0, 4)) * HOP
            t_s = (on0[n] + float(rs.uniform(-1, 1)) * tol / HOP) * HOP
            anchors.append((int(n), t_s, tol))
            f = [f for f in range(-5, T + 5) if abs(f * HOP - t_s) <= tol + 1e-12] + [int(math.floor(t_s / HOP + 0.5))]
            ranges[int(n)] = (max(min(f), ranges.get(int(n), (-9, 0))[0]), min(max(f), ranges.get(int(n), (0, 10 ** 6))[1]))
            assert ranges[int(n)][0] <= on0[n] <= ranges[int(n)][1]
        windows = []
        for n in rs.permutation(sung)[: int(rs.randint(0, 3))]:
            a, b = on0[n] - int(rs.randint(0, 4)), off0[n] + int(rs.randint(0, 4))
            windows.append((int(n), a * HOP, b * HOP))
        lo, hi = wfa(L, T, windows, anchors, HOP)
        on, off, _, status, path = wr.viterbi_windows(em, labels, lo, hi, sf, 0.5)
        assert status == wr.LA_OK, (case, anchors, windows)
        for n, (f_lo, f_hi) in ranges.items():
            if on[n] >= 0:
                assert f_lo <= on[n] <= f_hi, (case, n, on[n], f_lo, f_hi)
        for n, lo_s, hi_s in windows:
            if on[n] >= 0:
                assert lo_s - 1e-9 <= on[n] * HOP and off[n] * HOP <= hi_s + 1e-9, (case, n)
        # narrowing the lattice around the best path leaves the best path in it: the result is the unconstrained one
        assert (on, off) == (on0, off0), case
        # and an anchor off the truth moves the result: the first sung character two frames later than the DP put it
        n = sung[0]
        if off0[n] - on0[n] >= 3:
            lo, hi = wfa(L, T, None, [(n, (on0[n] + 2) * HOP, 0.0)], HOP)
            on2, _, _, st2, _ = wr.viterbi_windows(em, labels, lo, hi, sf, 0.5)
            if st2 == wr.LA_OK and on2[n] >= 0:
                assert on2[n] == on0[n] + 2
                n_moved += 1
    assert n_moved > 30


# ------------------------------------------------------------------------------------------------ 4. parse_lrc
def test_parse_lrc():
    from lyricalignment_amd.harness import parse_lrc
    text = "\n".join(["[ar:Somebody]", "[ti:A song]", "[offset:0]", "",
                      "[00:12.30]first line", "[01:02.345] second line ", "[00:40.00][02:10.5]chorus",
                      "[00:05.00]", "[00:01.00]before everything", "no tag here", "[00:50]whole seconds"])
    got = parse_lrc(text)
    assert [line for _, line in got] == ["before everything", "first line", "chorus", "whole seconds", "second line", "chorus"]
    assert [round(t, 6) for t, _ in got] == [1.0, 12.3, 40.0, 50.0, 62.345, 130.5]
    assert parse_lrc("") == [] and parse_lrc("[ar:x]\n[00:01.00]\n") == []


# ------------------------------------------------------------------------------------------------ 5. the planted repeated phrase
def _twice(rs):
    """A two-line sheet (3 + 2 characters, classes 1..5) over audio that holds the two lines TWICE: a first pass (frames 3..22, e.g. a
    backing vocal before the lead enters) whose cells are a little clearer (-0.1) than those of the second, true pass (frames 26..45,
    -0.5).  Silence is clear (-0.3) only where nothing is sung; elsewhere every cell is about -6, the silence column -3."""
    truth = [0] * 3 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0] * 3 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0] * 3
    T = len(truth)
    em = -6.0 + 0.2 * rs.randn(T, 6)
    em[:, 0] = -3.0
    for t, c in enumerate(truth):
        em[t, c] = -0.3 if c == 0 else (-0.1 if t < 24 else -0.5)
    return em.astype(np.float32), T


def test_a_repeated_phrase_lands_on_the_anchored_occurrence_and_the_next_line_moves_with_it():
    from lyricalignment_amd.utils.alignment import windows_from_anchors as wfa
    for seed in range(20):
        em, T = _twice(np.random.RandomState(300 + seed))
        labels = [1, 2, 3, 4, 5]
        lo, hi = wr.open_windows(5, T)
        on, off, _, status, _ = wr.viterbi_windows(em, labels, lo, hi)
        assert status == wr.LA_OK and on == [3, 7, 11, 15, 19]                          # without an anchor: the first, wrong occurrence
        lo, hi = wfa(5, T, onset_anchors=[(0, 26 * HOP + 0.013, 0.1)], hop_size_second=HOP)  # "the sheet says line 1 starts at 0.53 s"
        on, off, _, status, _ = wr.viterbi_windows(em, labels, lo, hi)
        assert status == wr.LA_OK
        assert on == [26, 30, 34, 38, 42] and off == [30, 34, 38, 42, 46]               # the right one, and line 2 (characters 3, 4) with it
    # an anchor past the clip's end: no path.  As for a clip too short for its labels, the -1e7 initial value of the states >= 2 at frame 0
    # can still carry a finite score to the end (the path then misses label 0): the status says it, and -inf only when row 0 is closed too
    lo, hi = wfa(5, T, onset_anchors=[(0, 2.0, 0.1)], hop_size_second=HOP)
    assert wr.enumerate_best(em, labels, lo, hi) is None
    on, off, score, status, _ = wr.viterbi_windows(em, labels, lo, hi)
    assert status == wr.LA_EINFEASIBLE and on[0] == -1 and score < wr.NEG
    assert wr.viterbi_windows(em, labels, [1] * 11, hi)[:4] == ([-1] * 5, [-1] * 5, wr.NINF, wr.LA_EINFEASIBLE)


# ------------------------------------------------------------------------------------------------ 6. the library's host face
def test_window_entry_points_are_declared_exported_and_check_arguments_on_the_host():
    from lyricalignment_amd import _lib
    text = open(os.path.join(ROOT, "include", "lyricalign.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("la_viterbi_windows_workspace_bytes", "la_viterbi_windows_batch"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in lyricalign.h"
        assert name in _lib.SYMBOLS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} not exported"
    L = _lib.lib()
    assert L.la_version() == 2
    need, need_spans = ctypes.c_size_t(1), ctypes.c_size_t(2)
    f = L.la_viterbi_windows_workspace_bytes
    for shape in ((32, 1500, 26), (2, 7000, 26), (3, 9000, 238), (1, 600, 511), (1, 40, 511)):            # the span planner's answers
        assert f(*shape, ctypes.byref(need)) == _lib.LA_OK
        assert L.la_viterbi_spans_workspace_bytes(*shape, ctypes.byref(need_spans)) == _lib.LA_OK and need.value == need_spans.value
    assert f(2, 7000, 26, ctypes.byref(need)) == _lib.LA_OK and need.value == 2 * 7000 * 1 * 24
    assert f(1, 600, 512, ctypes.byref(need)) == _lib.LA_EUNSUPPORTED and "511" in _lib.last_error()
    assert f(1, 600, 26, None) == _lib.LA_EINVAL

    P = 16                                      # a non-null, aligned stand-in pointer: every call below is refused before any device call
    big = 1 << 40

    def call(em=P, labels=P, n_labels=P, n_frames=P, batch=2, T=100, Lmax=26, onset=P, offset=P, out_stride=26, score=P, status=P,
             skip_from=P, skip_stride=27, penalty=0.0, win_lo=P, win_hi=P, win_stride=53, ws=P, ws_bytes=big, em_rs=27, labels_stride=26):
        return L.la_viterbi_windows_batch(em, T * em_rs, em_rs, labels, labels_stride, n_labels, n_frames, batch, T, Lmax, onset, offset,
                                          out_stride, score, status, skip_from, skip_stride, penalty, win_lo, win_hi, win_stride,
                                          ws, ws_bytes, 0)

    for null in ("em", "labels", "n_labels", "n_frames", "onset", "offset", "score", "status", "win_lo", "win_hi"):
        assert call(**{null: 0}) == _lib.LA_EINVAL, null
        assert "null" in _lib.last_error() and "viterbi_windows_batch" in _lib.last_error()
    assert call(win_stride=52) == _lib.LA_EINVAL and "strides" in _lib.last_error()                       # 2 * max_labels
    assert call(penalty=-0.5) == _lib.LA_EINVAL and "skip_penalty" in _lib.last_error()
    assert call(penalty=float("nan")) == _lib.LA_EINVAL and "skip_penalty" in _lib.last_error()
    assert call(skip_stride=26) == _lib.LA_EINVAL and "strides" in _lib.last_error()
    assert call(out_stride=25) == _lib.LA_EINVAL
    assert call(em_rs=26) == _lib.LA_EINVAL
    assert call(T=0) == _lib.LA_EINVAL
    assert call(Lmax=512, out_stride=512, em_rs=513, labels_stride=512, skip_stride=513, win_stride=1025) == _lib.LA_EUNSUPPORTED
    assert "511" in _lib.last_error()
    assert call(T=7000, ws_bytes=2 * 7000 * 24 - 1) == _lib.LA_EINVAL and "workspace too small" in _lib.last_error()
    assert call(T=7000, ws=0) == _lib.LA_EINVAL
    assert call(batch=0) == _lib.LA_OK          # nothing to do, nothing enqueued
