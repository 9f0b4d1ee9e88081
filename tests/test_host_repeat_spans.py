"""CPU-only checks of the alignment DP with repeatable lyric lines: the float64 yardstick (tests/repeat_spans_reference.py) against
tests/optional_spans_reference.py without repeat arcs and against exhaustive path enumeration with them, its row-vectorised form
against the plain one, the planted "A B B C" / "A B C B" sheets the feature exists for, the visits cut from a path, the
visit-beats-skip rule, the host helpers and the host face of la_viterbi_repeats_batch (declared, exported, planner, argument checks
answered before any device call)."""
import ctypes
import os
import re

import numpy as np
import pytest

import optional_spans_reference as osr
import repeat_spans_reference as rr
import windows_reference as wr
from conftest import ROOT
from test_host_optional_spans import _compact, _random_labels, _random_spans


def _random_repeats(rs, L, p=0.5):
    """repeat_from [L]: each start a gets a span with probability p, its end uniform in a+1 .. L; some entries are out-of-range junk
    (e <= a, e > L), which must read as "none"."""
    rf = [-1] * L
    for a in range(L):
        u = rs.rand()
        if u < p:
            rf[a] = int(rs.randint(a + 1, L + 1))
        elif u < p + 0.1:
            rf[a] = int(rs.choice([a, 0, L + 1, -5]))
            if a < rf[a] <= L:
                rf[a] = -1
    return rf


def _dyadic(rs, T, labels):
    """Compact emissions [T, L+1] float32 in steps of 1/4 (ties occur and every sum is exact), equal labels sharing a column."""
    V = max(labels)
    lp = (-rs.randint(0, 9, size=(T, V)) / 4.0).astype(np.float32)
    ls = (-rs.randint(0, 9, size=(T, 1)) / 4.0).astype(np.float32)
    return np.concatenate([ls, lp[:, np.asarray(labels) - 1]], axis=1)


# ------------------------------------------------------------------------------------------------ 1. no repeat arcs = the span lattice
def test_without_repeat_arcs_the_restatement_is_the_span_lattice_exactly():
    rs = np.random.RandomState(11)
    for case in range(200):
        T, L = int(rs.randint(1, 41)), int(rs.randint(1, 9))
        labels = _random_labels(rs, L)
        sf = _random_spans(rs, L) if case % 2 else [-1] * (L + 1)
        pen = 0.5 if case % 4 == 1 else 0.0
        em, _, _ = _compact(rs, T, labels)
        want = osr.viterbi_spans(em, labels, sf, pen)
        for rf in (None, [-1] * L, [a for a in range(L)], [L + 1] * L):               # null, the convention, and junk that is no span
            got = rr.viterbi(em, labels, sf, pen, rf, 0.25)
            assert tuple(got) == want, (case, rf)
            assert got.n_repeats == 0
        dp, bt, codes = rr.lattice(em, labels, sf, pen)
        dp_o, bt_o, jumped = osr.lattice(em, labels, sf, pen)
        assert dp == dp_o and bt[1:] == bt_o[1:]
        assert [[c in (3, 4) for c in row] for row in codes] == jumped
    # and with windows: the windowed restatement
    for case in range(60):
        T, L = int(rs.randint(2, 30)), int(rs.randint(1, 7))
        labels = _random_labels(rs, L)
        sf = _random_spans(rs, L)
        em, _, _ = _compact(rs, T, labels)
        lo = [int(rs.randint(0, 3)) if rs.rand() < 0.3 else 0 for _ in range(2 * L + 1)]
        hi = [T - int(rs.randint(0, 3)) if rs.rand() < 0.3 else T for _ in range(2 * L + 1)]
        assert tuple(rr.viterbi(em, labels, sf, 0.5, None, 0.0, lo, hi)) == wr.viterbi_windows(em, labels, lo, hi, sf, 0.5), case


# ------------------------------------------------------------------------------------------------ 2. exhaustive enumeration
def test_with_repeat_arcs_the_dp_equals_exhaustive_enumeration():
    """400 random lattices with L <= 3, T <= 7, dyadic emissions (ties occur), random repeat spans, half of them with optional spans too,
    penalties 0 / 0.5 / 0.25: on every case with a path the DP's score equals the best score over ALL lattice paths, accumulated in the
    same order, the reported path is a path of the lattice, and the status is LA_OK; without any path the status is LA_EINFEASIBLE (the
    score is then the ~ -1e7 artefact of the initial value and is not compared)."""
    rs = np.random.RandomState(5)
    n_feasible = n_repeat = n_both = 0
    for case in range(400):
        T, L = int(rs.randint(1, 8)), int(rs.randint(1, 4))
        labels = _random_labels(rs, L, 3)
        rf = _random_repeats(rs, L, 0.7)
        sf = _random_spans(rs, L) if case % 2 else None
        pen, rpen = (0.5, 0.25) if case % 3 == 0 else (0.0, 0.0) if case % 3 == 1 else (0.25, 0.5)
        em = _dyadic(rs, T, labels)
        want = rr.enumerate_best(em, labels, sf, pen, rf, rpen)
        got = rr.viterbi(em, labels, sf, pen, rf, rpen)
        on, off, score, status, path = got
        assert status == (rr.LA_OK if want is not None else rr.LA_EINFEASIBLE), (case, T, labels, sf, rf, path)
        if want is None:
            continue
        n_feasible += 1
        assert score == want, (case, T, labels, sf, rf)
        preds = rr.arcs(labels, sf, rf)
        assert path[0] in (0, 1) and path[-1] in (2 * L, 2 * L - 1)
        for t in range(1, T):
            assert path[t - 1] in [src for src, _ in preds[path[t]]] and not (path[t] == 0 and path[t - 1] != 0)
        for n in range(L):
            assert (on[n] < 0) == (2 * n + 1 not in path)
            if on[n] >= 0:
                assert on[n] == path.index(2 * n + 1)
        n_repeat += got.n_repeats > 0
        n_both += got.n_repeats > 0 and got.n_jumps > 0
        assert tuple(rr.viterbi(em, labels, sf, pen, rf, rpen, rows=True)) == tuple(got)
    print(f"{n_feasible} of 400 feasible, {n_repeat} take a repeat arc, {n_both} a repeat arc and a skip jump")
    assert n_feasible > 200 and n_repeat > 20 and n_both > 0


def test_the_row_vectorised_form_equals_the_plain_form_cell_by_cell():
    rs = np.random.RandomState(17)
    for case in range(60):
        T, L = int(rs.randint(2, 40)), int(rs.randint(1, 12))
        labels = _random_labels(rs, L, 3)
        rf, sf = _random_repeats(rs, L), _random_spans(rs, L)
        em = _dyadic(rs, T, labels) if case % 2 else _compact(rs, T, labels)[0]
        lo = [int(rs.randint(0, 3)) if rs.rand() < 0.2 else 0 for _ in range(2 * L + 1)]
        hi = [T - int(rs.randint(0, 3)) if rs.rand() < 0.2 else T for _ in range(2 * L + 1)]
        if case % 3 == 0:
            lo = hi = None
        a = rr.lattice(em, labels, sf, 0.25, rf, 0.5, lo, hi)
        b = rr.lattice_rows(em, labels, sf, 0.25, rf, 0.5, lo, hi)
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x)[1:], np.asarray(y)[1:]), case
        assert np.array_equal(np.asarray(a[0])[0], b[0][0])


# ------------------------------------------------------------------------------------------------ 3. the planted sheets
def _planted(rs, sung, n_labels, seg=4, noise=True):
    """Emissions for a sung sequence of label INDICES (each seg frames, a seg-frame silence between and around them): the sung cell -0.25,
    every other cell -6 minus dyadic noise."""
    truth = [0] * seg
    for n in sung:
        truth += [1 + n] * seg + [0] * seg
    T = len(truth)
    em = -6.0 - (rs.randint(0, 5, size=(T, n_labels + 1)) / 4.0 if noise else 0.0) * np.ones((T, n_labels + 1))
    for t, c in enumerate(truth):
        em[t, c] = -0.25
    return em.astype(np.float32), truth


def test_planted_abbc_and_abcb_sheets_are_recovered():
    """A sheet A B C (two labels per line) over audio that sings A B B C, and one that sings A B C B: with line B repeatable (A B B C),
    or a repeat span over B..C plus C optional (A B C B, the chorus that returns after the second verse), every visit is found where it
    was planted; without the repeat span the second chorus is forced onto silence or onto other lines (a lower score, another path)."""
    rs = np.random.RandomState(3)
    labels = [1, 2, 3, 4, 5, 6]                                   # A = 0, 1; B = 2, 3; C = 4, 5
    for sung, rf, sf in (([0, 1, 2, 3, 2, 3, 4, 5], [-1, -1, 4, -1, -1, -1], None),
                         ([0, 1, 2, 3, 4, 5, 2, 3], [-1, -1, 6, -1, -1, -1], [-1, -1, -1, -1, -1, -1, 4])):
        em, truth = _planted(rs, sung, 6)
        got = rr.viterbi(em, labels, sf, 0.0, rf, 1.0)
        assert got[3] == rr.LA_OK and got.n_repeats == 1
        assert [n for n, _, _ in rr.segments(got[4])] == sung
        assert [(first, end) for _, first, end in rr.segments(got[4])] == [(4 + 8 * i, 8 + 8 * i) for i in range(len(sung))]
        assert got[0] == [4 + 8 * sung.index(n) for n in range(6)]                 # the FIRST visit
        mono = rr.viterbi(em, labels, sf, 0.0, None, 0.0)
        assert mono.n_repeats == 0 and mono[2] < got[2] and mono[4] != got[4]
        # a penalty above what the repetition gains: the repeat-free result
        assert tuple(rr.viterbi(em, labels, sf, 0.0, rf, 1000.0)) == tuple(mono)


# ------------------------------------------------------------------------------------------------ 4. segments and the visit-beats-skip rule
def test_segments_cut_from_a_path():
    assert rr.segments([]) == []
    assert rr.segments([0, 0, 2, 2]) == []
    assert rr.segments([1, 1, 2, 3, 3, 3, 1, 4, 5]) == [(0, 0, 2), (1, 3, 6), (0, 6, 7), (2, 8, 9)]
    assert rr.segments([1, 3, 1, 3, -1, -1]) == [(0, 0, 1), (1, 1, 2), (0, 2, 3), (1, 3, 4)]


def test_a_label_skipped_on_one_pass_and_visited_on_another_has_its_visit():
    """Sheet A B C D with B optional and a repeat span over A..C; the audio sings A C A B C D: the first pass jumps over B, the second
    visits it.  B has the onset of its visit (not -1), the status is LA_OK, and the first-visit rule holds for A and C."""
    labels = [1, 2, 3, 4]
    sf = [-1, -1, 1, -1, -1]                                       # label 1 (B) optional
    rf = [3, -1, -1, -1]                                           # labels 0 .. 2 repeatable
    em, truth = _planted(np.random.RandomState(0), [0, 2, 0, 1, 2, 3], 4, noise=False)
    got = rr.viterbi(em, labels, sf, 0.0, rf, 0.0)
    assert [n for n, _, _ in rr.segments(got[4])] == [0, 2, 0, 1, 2, 3]
    assert got.n_jumps == 1 and got.n_repeats == 1 and got[3] == rr.LA_OK
    assert got[0] == [4, 28, 12, 44] and got[1] == [8, 32, 16, 48]


# ------------------------------------------------------------------------------------------------ 5. host helpers
def test_repeats_from_lines_and_span_validation():
    from lyricalignment_amd.utils.alignment import _repeat_from_of_spans, repeats_from_lines
    assert repeats_from_lines([2, 3, 1], [False, True, True]) == [-1, -1, 5, -1, -1, 6]
    assert repeats_from_lines([2], [False]) == [-1, -1]
    with pytest.raises(ValueError):
        repeats_from_lines([2, 3], [True])
    with pytest.raises(ValueError):
        repeats_from_lines([2, 0], [True, False])
    lists = [[1, 2, 3], [4, 5]]
    assert _repeat_from_of_spans(None, lists) is None
    assert _repeat_from_of_spans([[], None], lists) is None
    rows = _repeat_from_of_spans([[(0, 3), (1, 2)], [(1, 2)]], lists)
    assert rows.tolist() == [[3, 2, -1], [-1, 2, -1]] and str(rows.dtype) == "torch.int32"
    for bad in ([[(-1, 2)], []], [[(1, 1)], []], [[(2, 1)], []], [[(0, 4)], []], [[], [(0, 3)]], [[(0, 2), (0, 3)], []]):
        with pytest.raises(ValueError):
            _repeat_from_of_spans(bad, lists)
    with pytest.raises(ValueError):
        _repeat_from_of_spans([[]], lists)


def test_line_occurrences_of_the_harness():
    from lyricalignment_amd.harness import _line_occurrences
    seg = [(0, 0.0, 0.1), (1, 0.1, 0.2), (3, 0.3, 0.4), (3, 0.5, 0.6), (0, 0.7, 0.8), (1, 0.8, 0.9)]
    assert _line_occurrences(seg, ["ab", "c", "d"]) == [[[[0.0, 0.1, "a"], [0.1, 0.2, "b"]], [[0.7, 0.8, "a"], [0.8, 0.9, "b"]]], [],
                                                        [[[0.3, 0.4, "d"]], [[0.5, 0.6, "d"]]]]


# ------------------------------------------------------------------------------------------------ 6. the library's host face
def test_repeat_entry_points_are_declared_exported_and_check_arguments_on_the_host():
    from lyricalignment_amd import _lib
    text = open(os.path.join(ROOT, "include", "lyricalign.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("la_viterbi_repeats_workspace_bytes", "la_viterbi_repeats_batch"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in lyricalign.h"
        assert name in _lib.SYMBOLS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} not exported"
    L = _lib.lib()
    need, need_lattice = ctypes.c_size_t(1), ctypes.c_size_t(2)
    f = L.la_viterbi_repeats_workspace_bytes
    for shape in ((32, 1500, 26), (2, 7000, 26), (3, 9000, 238), (1, 600, 511), (1, 600, 512), (1, 12000, 2500), (2, 50, 4095)):
        assert f(*shape, ctypes.byref(need)) == _lib.LA_OK
        assert L.la_viterbi_lattice_workspace_bytes(*shape, ctypes.byref(need_lattice)) == _lib.LA_OK and need.value == need_lattice.value
    assert f(1, 600, 4096, ctypes.byref(need)) == _lib.LA_EUNSUPPORTED and "4095" in _lib.last_error()
    assert f(1, 600, 26, None) == _lib.LA_EINVAL

    P = 16                                      # a non-null, aligned stand-in pointer: every call below is refused before any device call
    big = 1 << 40

    def call(em=P, labels=P, n_labels=P, n_frames=P, batch=2, T=100, Lmax=26, onset=P, offset=P, out_stride=26, score=P, status=P,
             skip_from=P, skip_stride=27, penalty=0.0, win_lo=P, win_hi=P, win_stride=53, repeat_from=P, repeat_stride=26,
             repeat_penalty=0.0, path=P, path_stride=100, ws=P, ws_bytes=big, em_rs=27, labels_stride=26):
        return L.la_viterbi_repeats_batch(em, T * em_rs, em_rs, labels, labels_stride, n_labels, n_frames, batch, T, Lmax, onset, offset,
                                          out_stride, score, status, skip_from, skip_stride, penalty, win_lo, win_hi, win_stride,
                                          repeat_from, repeat_stride, repeat_penalty, path, path_stride, ws, ws_bytes, 0)

    for null in ("em", "labels", "n_labels", "n_frames", "onset", "offset", "score", "status"):
        assert call(**{null: 0}) == _lib.LA_EINVAL, null
        assert "null" in _lib.last_error() and "viterbi_repeats_batch" in _lib.last_error()
    assert call(win_lo=0) == _lib.LA_EINVAL and "go together" in _lib.last_error()
    assert call(win_hi=0) == _lib.LA_EINVAL and "go together" in _lib.last_error()
    assert call(win_stride=52) == _lib.LA_EINVAL and "strides" in _lib.last_error()
    assert call(skip_stride=26) == _lib.LA_EINVAL and "strides" in _lib.last_error()
    assert call(penalty=-0.5) == _lib.LA_EINVAL and "skip_penalty" in _lib.last_error()
    assert call(repeat_penalty=-0.5) == _lib.LA_EINVAL and "repeat_penalty" in _lib.last_error()
    assert call(repeat_penalty=float("nan")) == _lib.LA_EINVAL and "repeat_penalty" in _lib.last_error()
    assert call(repeat_stride=25) == _lib.LA_EINVAL and "repeat_stride" in _lib.last_error()
    assert call(path_stride=99) == _lib.LA_EINVAL and "path_stride" in _lib.last_error()
    assert call(out_stride=25) == _lib.LA_EINVAL
    assert call(em_rs=26) == _lib.LA_EINVAL
    assert call(T=0) == _lib.LA_EINVAL
    assert call(Lmax=4096, out_stride=4096, em_rs=4097, labels_stride=4096, skip_stride=4097, win_stride=8193, repeat_stride=4096) == _lib.LA_EUNSUPPORTED
    assert "4095" in _lib.last_error()
    assert call(T=7000, path_stride=7000, ws_bytes=2 * 7000 * 24 - 1) == _lib.LA_EINVAL and "workspace too small" in _lib.last_error()
    assert call(T=7000, path_stride=7000, ws=0) == _lib.LA_EINVAL
    assert call(batch=0) == _lib.LA_OK          # nothing to do, nothing enqueued
