"""CPU-only checks of the confidence for anchored alignment (posteriors on the lattice with per-state frame windows): the float64 yardstick
tests/window_posterior_reference.py against exhaustive enumeration of the paths inside the windows and against
tests/span_posterior_reference.py with open windows, the non-vacuity of the window sets that tests/test_gpu_window_posteriors.py hands
to the kernel, and the host face of la_alignment_posteriors_windows (declared, exported, argument checks answered before any device call)."""
import ctypes
import os
import re

import numpy as np
import pytest

import span_posterior_reference as spr
import window_posterior_reference as wpr
import windows_reference as wr
from conftest import ROOT


def _em(rs, T, labels, lean=0.0):
    """Compact emissions [T, L+1] in -3 .. 0 (label columns lowered by lean); equal labels carry identical columns."""
    V = max(labels)
    lp = -rs.rand(T, V) * 3 - lean
    ls = -rs.rand(T, 1) * 3
    return np.concatenate([ls, lp[:, np.asarray(labels) - 1]], axis=1).astype(np.float32)


def _random_spans(rs, L, p=0.5):
    sf = [-1] * (L + 1)
    for n in range(1, L + 1):
        if rs.rand() < p:
            sf[n] = int(rs.randint(0, n))
    return sf


def _against_enumeration(em, labels, lo, hi, sf, pen, what):
    """-> True when a path exists: gamma, log_z, present and span_skip equal the enumeration's, rows sum to 1, gamma is exactly 0 outside."""
    T, L = em.shape[0], len(labels)
    gamma, entry, exit_, present, span_skip, log_z = wpr.posteriors(em, labels, lo, hi, sf, pen)
    want = wpr.brute(em, labels, lo, hi, sf, pen)
    if want is None:
        assert np.isneginf(log_z) and not gamma.any() and not entry.any() and not exit_.any() and not present.any() and not span_skip.any(), what
        return False
    g_b, lz_b, pres_b, skip_b = want
    assert abs(log_z - lz_b) <= 1e-12 and np.abs(gamma - g_b).max() <= 1e-12, (what, log_z, lz_b)
    assert np.abs(present - pres_b).max() <= 1e-12 and np.abs(span_skip - skip_b).max() <= 1e-12, what
    assert np.abs(gamma.sum(1) - 1).max() <= 1e-12, what
    assert not gamma[~wpr.inside(T, 2 * L + 1, lo, hi)].any(), what                      # exactly 0 outside the windows
    assert np.abs(entry.sum(0) - exit_.sum(0)).max() <= 1e-12, what                      # a label that is entered is left
    cov = spr.coverage(present, span_skip, sf if sf is not None else [-1] * (L + 1))
    assert np.abs(cov - 1).max() <= 1e-12, what
    return True


# ------------------------------------------------------------------------------------------------ 1. the yardstick against enumeration
def test_yardstick_equals_enumeration_of_the_paths_inside_the_windows():
    """400 random lattices (T <= 10, L <= 4, half with spans, penalties 0 / 0.5 / 1, about a third of the states with a random lo and a
    third with a random hi), then the named edges."""
    rs = np.random.RandomState(0)
    feasible = with_spans = 0
    for case in range(400):
        L = int(rs.randint(1, 5))
        T = int(rs.randint(1, 11 if L <= 3 else 9))
        labels = [int(v) for v in rs.randint(1, 4, size=L)]
        sf = _random_spans(rs, L) if case % 2 else None
        pen = (0.0, 0.5, 1.0)[case % 3]
        em = _em(rs, T, labels, lean=1.0 * (case % 2))
        S = 2 * L + 1
        lo = [int(rs.randint(0, T + 1)) if rs.rand() < 0.3 else 0 for _ in range(S)]
        hi = [int(rs.randint(0, T + 1)) if rs.rand() < 0.3 else T for _ in range(S)]
        ok = _against_enumeration(em, labels, lo, hi, sf, pen, (case, T, labels, sf, lo, hi))
        feasible += ok
        with_spans += ok and sf is not None
    print(f"{feasible} of 400 cases with a path, {with_spans} of them with spans")
    assert 100 < feasible < 350 and with_spans > 50


def test_yardstick_on_the_named_edges_and_the_issue_lattice():
    """A repeated neighbour pair under windows; state 0 closed at frame 0 (gamma[0, 1] = 1); state S-1 closed at frame T-1 (the path ends in
    S-2); the 9-frame, 3-label lattice with a span and a repeated pair: the windows leave undecided cells and a window_log_prob below 0."""
    rs = np.random.RandomState(3)
    T, labels = 9, [2, 2, 1]
    S = 7
    em = _em(rs, T, labels)
    for sf in (None, [-1, -1, 0, 1]):
        for pen in (0.0, 1.0):
            o_lo, o_hi = wr.open_windows(3, T)
            lo, hi = list(o_lo), list(o_hi)
            lo[0] = 1
            assert _against_enumeration(em, labels, lo, hi, sf, pen, "state 0 closed at frame 0")
            gamma = wpr.posteriors(em, labels, lo, hi, sf, pen)[0]
            assert gamma[0, 0] == 0.0 and abs(gamma[0, 1] - 1) <= 1e-12
            lo, hi = list(o_lo), list(o_hi)
            hi[S - 1] = T - 1
            assert _against_enumeration(em, labels, lo, hi, sf, pen, "state S-1 closed at frame T-1")
            gamma = wpr.posteriors(em, labels, lo, hi, sf, pen)[0]
            assert gamma[T - 1, S - 1] == 0.0 and abs(gamma[T - 1, S - 2] - 1) <= 1e-12
            # the repeated pair (labels 0 and 1 are equal: no arc 1 -> 3) under windows on both of its states and the silence between
            lo, hi = list(o_lo), list(o_hi)
            lo[1], hi[1], lo[2], hi[2], lo[3], hi[3] = 0, 4, 1, 6, 2, 8
            assert _against_enumeration(em, labels, lo, hi, sf, pen, "repeated pair")
            gamma, _, _, _, _, log_z = wpr.posteriors(em, labels, lo, hi, sf, pen)
            free = spr.posteriors(em, labels, sf if sf is not None else [-1] * 4, pen)[5]
            undecided = int(((gamma > 0.05) & (gamma < 0.95)).sum())
            print(f"spans={sf is not None} penalty={pen}: window_log_prob {log_z - free:.3f}, {undecided} undecided cells")
            assert log_z - free < -1e-3 and undecided >= 5


# ------------------------------------------------------------------------------------------------ 2. open windows, no path
def test_open_windows_equal_the_span_yardstick_exactly_and_no_path_gives_zeros():
    rs = np.random.RandomState(5)
    for case in range(40):
        L = int(rs.randint(1, 12))
        T = int(rs.randint(L + 2, 40))
        labels = [int(v) for v in rs.randint(1, 5, size=L)]
        sf = _random_spans(rs, L, 0.3) if case % 2 else [-1] * (L + 1)
        em = _em(rs, T, labels, lean=1.0)
        lo, hi = wr.open_windows(L, T)
        if case % 4 == 0:                                   # any int32 pair that covers [0, T) is an open window
            lo, hi = [-3] * len(lo), [T + 5] * len(hi)
        got = wpr.posteriors(em, labels, lo, hi, sf if case % 2 else None, 0.5)
        want = spr.posteriors(em, labels, sf, 0.5)
        for g, w in zip(got, want):
            assert np.array_equal(np.asarray(g), np.asarray(w)), case
        # a label with lo == hi, and every state closed at frame 0: no path
        S = 2 * L + 1
        for lo2, hi2 in (([0] * 1 + [7] + [0] * (S - 2), [T] + [7] + [T] * (S - 2)), ([1] * S, [T] * S)):
            dead = wpr.posteriors(em, labels, lo2, hi2, [-1] * (L + 1), 0.5)
            assert np.isneginf(dead[5]) and not any(np.asarray(x).any() for x in dead[:5]), case


# ------------------------------------------------------------------------------------------------ 3. the device test is not vacuous
@pytest.mark.parametrize("T,L", wpr.GPU_SHAPES, ids=[f"T{t}_L{l}" for t, l in wpr.GPU_SHAPES])
def test_the_window_sets_of_the_device_test_have_a_path_and_move_gamma(T, L):
    """Every window set of tests/test_gpu_window_posteriors.py's shape cases: log_z finite, and gamma differs from the unwindowed gamma by
    more than 0.5 somewhere.  (The span-free lattice of 511 labels in 300 frames has no path under any windows: it must be the one
    infeasible entry, with open windows.)"""
    n = 0
    for skip, pen, lab, ems, los, his, refs, feasible in wpr.gpu_cases(T, L):
        assert feasible == (not ((T, L) == (300, 511) and skip is None))
        for c in range(2):
            gamma, log_z = refs[c][0], refs[c][5]
            if not feasible:
                assert np.isneginf(log_z) and (los[c], his[c]) == wr.open_windows(L, T)
                continue
            free = spr.posteriors(ems[c], lab, skip if skip is not None else [-1] * (L + 1), pen)
            moved = float(np.abs(gamma - free[0]).max())
            undecided = int(((gamma > 0.05) & (gamma < 0.95)).sum())
            print(f"T={T} L={L} spans={skip is not None} penalty={pen} clip {c}: log_z {log_z:.2f} (free {free[5]:.2f}), "
                  f"max |gamma - free gamma| {moved:.4f}, {undecided} undecided cells")
            assert np.isfinite(log_z) and log_z <= free[5] and moved > 0.5
            assert np.abs(gamma.sum(1) - 1).max() <= 1e-9
            n += 1
    assert n >= 2


def test_the_edge_window_sets_of_the_device_test_have_a_path():
    narrowed = 0
    for T, L in wpr.EDGE_SHAPES:
        for skip, pen, lab, em, lo, hi, ref, feasible in wpr.edge_cases(T, L):
            assert np.isfinite(ref[5]) == feasible, (T, L, skip)
            if feasible:
                assert np.abs(ref[0].sum(1) - 1).max() <= 1e-12
                narrowed += any(a > 0 or b < T for a, b in zip(lo, hi))
    assert narrowed >= 20              # (a state that holds the path for the whole clip narrows nothing: the one-label clips of a few frames)


# ------------------------------------------------------------------------------------------------ 4. the library's host face
def test_window_posterior_entry_points_are_declared_exported_and_check_arguments_on_the_host():
    from lyricalignment_amd import _lib
    text = open(os.path.join(ROOT, "include", "lyricalign.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("la_alignment_posteriors_windows_workspace_bytes", "la_alignment_posteriors_windows"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in lyricalign.h"
        assert name in _lib.SYMBOLS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} not exported"
    L = _lib.lib()
    assert L.la_version() == 2
    need, need_spans = ctypes.c_size_t(1), ctypes.c_size_t(2)
    f = L.la_alignment_posteriors_windows_workspace_bytes
    for shape in ((32, 1500, 26), (2, 7000, 26), (3, 9000, 238), (1, 600, 511), (1, 40, 511)):            # the spans query's answers
        assert f(*shape, ctypes.byref(need)) == _lib.LA_OK
        assert L.la_alignment_posteriors_spans_workspace_bytes(*shape, ctypes.byref(need_spans)) == _lib.LA_OK and need.value == need_spans.value
    assert f(2, 100, 26, ctypes.byref(need)) == _lib.LA_OK and need.value == 2 * 100 * 64 * 8
    assert f(1, 600, 512, ctypes.byref(need)) == _lib.LA_EUNSUPPORTED and "511" in _lib.last_error()
    assert f(1, 600, 26, None) == _lib.LA_EINVAL

    P = 16                                      # a non-null, aligned stand-in pointer: every call below is refused before any device call
    big = 1 << 40

    def call(em=P, labels=P, n_labels=P, n_frames=P, batch=2, T=100, Lmax=26, onset=P, offset=P, out_stride=26, window=2, skip_from=P,
             skip_stride=27, penalty=0.0, win_lo=P, win_hi=P, win_stride=53, occ=P, onp=P, offp=P, pres=P, skp=P, log_z=P, status=P, gamma=0,
             gamma_bs=0, gamma_rs=0, ws=P, ws_bytes=big, em_rs=27, labels_stride=26):
        return L.la_alignment_posteriors_windows(em, T * em_rs, em_rs, labels, labels_stride, n_labels, n_frames, batch, T, Lmax, onset, offset,
                                                 out_stride, window, skip_from, skip_stride, penalty, win_lo, win_hi, win_stride, occ, onp, offp,
                                                 pres, skp, log_z, status, gamma, gamma_bs, gamma_rs, ws, ws_bytes, 0)

    for null in ("em", "labels", "n_labels", "n_frames", "onset", "offset", "win_lo", "win_hi", "occ", "onp", "offp", "pres", "skp", "log_z",
                 "status"):
        assert call(**{null: 0}) == _lib.LA_EINVAL, null
        assert "null" in _lib.last_error() and "alignment_posteriors_windows" in _lib.last_error()
    assert call(win_stride=52) == _lib.LA_EINVAL and "strides" in _lib.last_error()                       # 2 * max_labels
    assert call(penalty=-0.5) == _lib.LA_EINVAL and "skip_penalty" in _lib.last_error()
    assert call(penalty=float("nan")) == _lib.LA_EINVAL and "skip_penalty" in _lib.last_error()
    assert call(skip_stride=26) == _lib.LA_EINVAL and "strides" in _lib.last_error()
    assert call(skip_from=0, skip_stride=26) == _lib.LA_EINVAL and "strides" in _lib.last_error()         # (span_skip_prob's row pitch)
    assert call(out_stride=25) == _lib.LA_EINVAL
    assert call(em_rs=26) == _lib.LA_EINVAL
    assert call(T=0) == _lib.LA_EINVAL
    assert call(window=-1) == _lib.LA_EINVAL and "boundary_window" in _lib.last_error()
    assert call(gamma=P, gamma_bs=100 * 53, gamma_rs=52) == _lib.LA_EINVAL and "gamma" in _lib.last_error()
    assert call(Lmax=512, out_stride=512, em_rs=513, labels_stride=512, skip_stride=513, win_stride=1025) == _lib.LA_EUNSUPPORTED
    assert "511" in _lib.last_error()
    assert call(ws_bytes=2 * 100 * 64 * 8 - 1) == _lib.LA_EINVAL and "workspace too small" in _lib.last_error()
    assert call(ws=0) == _lib.LA_EINVAL
    assert call(ws=P + 4) == _lib.LA_EINVAL and "aligned" in _lib.last_error()
    assert call(batch=0) == _lib.LA_OK          # nothing to do, nothing enqueued
