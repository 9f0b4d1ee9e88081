"""CPU-only checks of the alignment DP with optional lyric lines: the float64 yardstick (tests/optional_spans_reference.py) against
oracle/viterbi_python.py without spans and against exhaustive path enumeration with them, the planted-line property the feature exists
for, the host helpers (spans_from_lines, span validation) and the host face of la_viterbi_spans_batch (declared, exported, planner,
argument checks answered before any device call)."""
import ctypes
import os
import re

import numpy as np
import pytest

import optional_spans_reference as osr
from conftest import ROOT


def _random_spans(rs, L, p=0.5):
    """skip_from [L+1]: each end position n >= 1 gets a span with probability p, its start uniform in 0..n-1."""
    sf = [-1] * (L + 1)
    for n in range(1, L + 1):
        if rs.rand() < p:
            sf[n] = int(rs.randint(0, n))
    return sf


def _random_labels(rs, L, n_classes=4):
    return [int(v) for v in rs.randint(1, n_classes + 1, size=L)]          # few classes: equal neighbours are common


def _compact(rs, T, labels, scale=4.0):
    """Compact emissions [T, L+1] float32 with equal labels carrying identical columns (one class column each)."""
    V = max(labels)
    lp = (-rs.rand(T, V) * scale).astype(np.float32)
    ls = (-rs.rand(T, 1) * scale).astype(np.float32)
    return np.concatenate([ls, lp[:, np.asarray(labels) - 1]], axis=1), lp, ls


# ------------------------------------------------------------------------------------------------ 1. no spans = the reference's DP
def test_without_spans_the_reference_is_the_oracle_lattice_and_backtrace():
    """200 random cases, T in 1..40, L in 1..8, repeated labels included: dp and bt equal oracle.viterbi_python.viterbi_lattice's cell by
    cell (== on float64), and onset / offset / status equal the reference's backtrace (path from the better of the last two states, first
    and last index of every label state; a label state that is missing is the reference's ValueError = LA_EINFEASIBLE)."""
    from oracle.viterbi_python import viterbi_lattice
    rs = np.random.RandomState(2024)
    n_infeasible = 0
    for case in range(200):
        T, L = int(rs.randint(1, 41)), int(rs.randint(1, 9))
        labels = _random_labels(rs, L)
        em, lp, ls = _compact(rs, T, labels)
        dp_o, bt_o = viterbi_lattice(lp, ls, np.asarray(labels))
        dp, bt, jumped = osr.lattice(em, labels, [-1] * (L + 1))
        assert np.array_equal(np.asarray(dp), dp_o), case
        assert np.array_equal(np.asarray(bt)[1:], bt_o[1:]), case
        assert not np.asarray(jumped).any()
        S = 2 * L + 1
        k = S - 1 if dp_o[-1][-1] > dp_o[-1][-2] else S - 2
        want_score = dp_o[-1][k]
        path = [k]
        for t in range(T - 1, 0, -1):
            k = int(bt_o[t][k])
            path.append(k)
        path.reverse()
        on, off, score, status, got_path = osr.viterbi_spans(em, labels, [-1] * (L + 1))
        assert got_path == path and score == want_score
        missing = [n for n in range(L) if 2 * n + 1 not in path]
        if missing:
            n_infeasible += 1
            assert status == osr.LA_EINFEASIBLE
        else:
            assert status == osr.LA_OK
            assert on == [path.index(2 * n + 1) for n in range(L)]
            assert off == [T - path[::-1].index(2 * n + 1) for n in range(L)]
    print(f"{n_infeasible} of 200 cases infeasible (T too short for the labels)")
    assert 0 < n_infeasible < 100


# ------------------------------------------------------------------------------------------------ 2. exhaustive enumeration
def test_score_equals_exhaustive_enumeration_of_lattice_paths():
    """300 random cases with T <= 6, L <= 4, random spans, penalties 0 and 0.5: the DP's score == the best score over ALL lattice paths,
    accumulated in the same order.  Cases without any path are left out (at most a quarter); in the others the reported path is a path of
    the lattice, its skipped labels are exactly the unvisited ones, and the status is LA_OK."""
    rs = np.random.RandomState(7)
    left_out = 0
    n_jumps = 0
    for case in range(300):
        T, L = int(rs.randint(1, 7)), int(rs.randint(1, 5))
        labels = _random_labels(rs, L, 3)
        sf = _random_spans(rs, L)
        pen = 0.5 if case % 2 else 0.0
        em, _, _ = _compact(rs, T, labels)
        want = osr.enumerate_best(em, labels, sf, pen)
        if want is None:
            left_out += 1
            continue
        on, off, score, status, path = osr.viterbi_spans(em, labels, sf, pen)
        assert score == want, (case, T, labels, sf, pen)
        assert status == osr.LA_OK, (case, T, labels, sf, path)
        preds = osr.arcs(labels, sf)
        assert path[0] in (0, 1) and path[-1] in (2 * L, 2 * L - 1)
        for t in range(1, T):
            assert path[t - 1] in [src for src, _ in preds[path[t]]] and not (path[t] == 0 and path[t - 1] != 0)
        for n in range(L):
            assert (on[n] < 0) == (2 * n + 1 not in path)
        n_jumps += any(o < 0 for o in on)
    print(f"{left_out} of 300 cases without a path; {n_jumps} reported paths take a jump")
    assert left_out <= 75
    assert n_jumps >= 30


# ------------------------------------------------------------------------------------------------ 3. planted lines
def _planted(rs, line_lengths, present, gap):
    """Audio of the lines with present[i]: 3 silence frames, every character of a present line for 4 frames, `gap` silence frames
    between present lines, 3 silence frames.  Truth cell about -0.3 +- 0.1, every other cell about -6 +- 1.  -> compact em [T, L+1]
    over ALL lines' characters (distinct classes)."""
    L = sum(line_lengths)
    truth = [0] * 3
    pos = 0
    first = True
    for n_chars, here in zip(line_lengths, present):
        if here:
            if not first:
                truth += [0] * gap
            first = False
            for n in range(pos, pos + n_chars):
                truth += [1 + n] * 4
        pos += n_chars
    truth += [0] * 3
    T = len(truth)
    em = -6.0 + rs.randn(T, L + 1)
    em[np.arange(T), truth] = -0.3 + 0.1 * rs.randn(T)
    return em.astype(np.float32)


def _check_planted(rs, line_lengths, optional, present, gap):
    from lyricalignment_amd.utils.alignment import spans_from_lines
    L = sum(line_lengths)
    labels = list(range(1, L + 1))
    em = _planted(rs, line_lengths, present, gap)
    on, off, score, status, _ = osr.viterbi_spans(em, labels, spans_from_lines(line_lengths, optional))
    assert status == osr.LA_OK
    starts = np.concatenate([[0], np.cumsum(line_lengths)])
    kept_lines = [all(on[n] >= 0 for n in range(starts[i], starts[i + 1])) for i in range(len(line_lengths))]
    gone_lines = [all(on[n] < 0 for n in range(starts[i], starts[i + 1])) for i in range(len(line_lengths))]
    assert [k != g for k, g in zip(kept_lines, gone_lines)] == [True] * len(line_lengths)        # a line is kept or left out as a whole
    assert kept_lines == [bool(v) for v in present]
    kept = [n for i in range(len(line_lengths)) if present[i] for n in range(starts[i], starts[i + 1])]
    true_on, true_off, true_score, true_status, _ = osr.viterbi_spans(em[:, [0] + [1 + n for n in kept]], [labels[n] for n in kept],
                                                                     [-1] * (len(kept) + 1))
    assert true_status == osr.LA_OK
    assert [on[n] for n in kept] == true_on and [off[n] for n in kept] == true_off
    return score, true_score, on, true_on, em, labels


def test_a_line_that_is_not_sung_is_left_out_and_its_neighbours_keep_their_frames():
    """Three lines of 3 / 4 / 3 characters, the middle one optional and absent, 50 seeds: the DP leaves exactly that line out, the other
    two lines' frames equal those from aligning the true lyrics, and the float64 path score is bit-equal.  Forcing the absent line (no
    spans: today's lattice) moves the other lines' onsets in most clips."""
    forced_equal = 0
    for seed in range(50):
        rs = np.random.RandomState(1000 + seed)
        score, true_score, on, true_on, em, labels = _check_planted(rs, [3, 4, 3], [False, True, False], [1, 0, 1], 2)
        assert score == true_score
        f_on, _, _, f_status, _ = osr.viterbi_spans(em, labels, [-1] * 11)
        forced_equal += f_status == osr.LA_OK and [f_on[n] for n in (0, 1, 2, 7, 8, 9)] == true_on
    print(f"forced alignment keeps the other two lines' onsets in {forced_equal} of 50 clips; with the span 50 of 50")
    assert forced_equal < 25


@pytest.mark.parametrize("gap", [0, 2])
@pytest.mark.parametrize("present", [(1, 1, 1, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 0, 1, 0)],
                         ids=lambda v: "".join(map(str, v)))
def test_all_lines_optional_reports_exactly_the_lines_that_were_synthesised(present, gap):
    """3 / 4 / 3 / 2 characters, all four lines optional, 30 seeds per presence pattern and gap: first line absent (one frame of the
    leading silence), last line absent (a span ending at L), two lines absent."""
    for seed in range(30):
        rs = np.random.RandomState(5000 + 100 * gap + seed)
        _check_planted(rs, [3, 4, 3, 2], [True] * 4, present, gap)


def test_two_adjacent_lines_left_out_together_cost_one_silence_frame_between_them():
    """Lines 2 and 3 of four absent: the path passes through the silence state between the two spans.  With 2 silence frames between the
    sung lines that frame is there and the result is the true lyrics'; with none the DP has to take one frame from a neighbour (the rule
    INTEGRATION.md states), so exactly one boundary of the kept lines moves by one frame."""
    for seed in range(30):
        _check_planted(np.random.RandomState(9000 + seed), [3, 4, 3, 2], [True] * 4, (1, 0, 0, 1), 2)
    from lyricalignment_amd.utils.alignment import spans_from_lines
    for seed in range(30):
        em = _planted(np.random.RandomState(9100 + seed), [3, 4, 3, 2], (1, 0, 0, 1), 0)
        on, off, _, status, path = osr.viterbi_spans(em, list(range(1, 13)), spans_from_lines([3, 4, 3, 2], [True] * 4))
        assert status == osr.LA_OK and [n for n in range(12) if on[n] < 0] == list(range(3, 10))
        assert path.count(2 * 7) == 1                                       # one frame in the silence between the two spans
        kept = [0, 1, 2, 10, 11]
        t_on, t_off, _, _, _ = osr.viterbi_spans(em[:, [0, 1, 2, 3, 11, 12]], [1, 2, 3, 11, 12], [-1] * 6)
        moved = sum(a != b for a, b in zip([on[n] for n in kept] + [off[n] for n in kept], t_on + t_off))
        assert moved == 1                                                   # label 2's offset or label 10's onset: the frame given to that silence


# ------------------------------------------------------------------------------------------------ 4. host helpers
def test_spans_from_lines_and_span_validation():
    from lyricalignment_amd.utils.alignment import _skip_from_of_spans, spans_from_lines
    assert spans_from_lines([3, 4, 3], [False, True, False]) == [-1, -1, -1, -1, -1, -1, -1, 3, -1, -1, -1]
    assert spans_from_lines([3, 4, 3, 2], [True] * 4) == [-1, -1, -1, 0, -1, -1, -1, 3, -1, -1, 7, -1, 10]
    assert spans_from_lines([2], [False]) == [-1, -1, -1]
    with pytest.raises(ValueError):
        spans_from_lines([3, 4], [True])
    with pytest.raises(ValueError):
        spans_from_lines([3, 0], [True, True])
    lists = [[5, 6, 7, 8], [9, 9]]
    assert _skip_from_of_spans(None, lists) is None
    assert _skip_from_of_spans([[], []], lists) is None
    rows = _skip_from_of_spans([[(0, 2), (2, 4)], [(1, 2)]], lists)
    assert rows.tolist() == [[-1, -1, 0, -1, 2], [-1, -1, 1, -1, -1]]
    for bad in ([[(-1, 2)], []], [[(2, 2)], []], [[(3, 1)], []], [[], [(0, 3)]], [[(0, 2), (1, 2)], []], [[(0, 1)]]):
        with pytest.raises(ValueError):
            _skip_from_of_spans(bad, lists)


# ------------------------------------------------------------------------------------------------ 5. / 6. the library's host face
def test_span_entry_points_are_declared_exported_and_check_arguments_on_the_host():
    from lyricalignment_amd import _lib
    text = open(os.path.join(ROOT, "include", "lyricalign.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("la_viterbi_spans_workspace_bytes", "la_viterbi_spans_batch"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in lyricalign.h"
        assert name in _lib.SYMBOLS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} not exported"
    L = _lib.lib()
    assert L.la_version() == 2
    need = ctypes.c_size_t(1)
    f = L.la_viterbi_spans_workspace_bytes
    assert f(32, 1500, 26, ctypes.byref(need)) == _lib.LA_OK and need.value == 0            # 1500 * 24 B of masks sit in LDS
    assert f(2, 7000, 26, ctypes.byref(need)) == _lib.LA_OK and need.value == 2 * 7000 * 1 * 24
    assert f(3, 9000, 238, ctypes.byref(need)) == _lib.LA_OK and need.value == 3 * 9000 * 8 * 24
    assert f(1, 600, 511, ctypes.byref(need)) == _lib.LA_OK and need.value == 600 * 16 * 24
    assert f(1, 40, 511, ctypes.byref(need)) == _lib.LA_OK and need.value == 0
    assert f(1, 600, 512, ctypes.byref(need)) == _lib.LA_EUNSUPPORTED and "511" in _lib.last_error()
    assert f(1, 600, 26, None) == _lib.LA_EINVAL
    with pytest.raises(NotImplementedError):
        _lib.check(f(1, 600, 512, ctypes.byref(need)), "x")

    P = 16                                      # a non-null, aligned stand-in pointer: every call below is refused before any device call
    big = 1 << 40

    def call(em=P, labels=P, n_labels=P, n_frames=P, batch=2, T=100, Lmax=26, onset=P, offset=P, out_stride=26, score=P, status=P,
             skip_from=P, skip_stride=27, penalty=0.0, ws=P, ws_bytes=big, em_rs=27, labels_stride=26):
        return L.la_viterbi_spans_batch(em, T * em_rs, em_rs, labels, labels_stride, n_labels, n_frames, batch, T, Lmax, onset, offset,
                                        out_stride, score, status, skip_from, skip_stride, penalty, ws, ws_bytes, 0)

    for null in ("em", "labels", "n_labels", "n_frames", "onset", "offset", "score", "status", "skip_from"):
        assert call(**{null: 0}) == _lib.LA_EINVAL, null
        assert "null" in _lib.last_error()
    assert call(penalty=-0.5) == _lib.LA_EINVAL and "skip_penalty" in _lib.last_error()
    assert call(penalty=float("nan")) == _lib.LA_EINVAL and "skip_penalty" in _lib.last_error()
    assert call(skip_stride=26) == _lib.LA_EINVAL and "strides" in _lib.last_error()
    assert call(out_stride=25) == _lib.LA_EINVAL
    assert call(em_rs=26) == _lib.LA_EINVAL
    assert call(T=0) == _lib.LA_EINVAL
    assert call(Lmax=512, out_stride=512, em_rs=513, labels_stride=512, skip_stride=513) == _lib.LA_EUNSUPPORTED and "511" in _lib.last_error()
    assert call(T=7000, ws_bytes=2 * 7000 * 24 - 1) == _lib.LA_EINVAL and "workspace too small" in _lib.last_error()
    assert call(T=7000, ws=0) == _lib.LA_EINVAL
    assert call(batch=0) == _lib.LA_OK          # nothing to do, nothing enqueued
