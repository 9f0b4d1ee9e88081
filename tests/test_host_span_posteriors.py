"""CPU-only checks of the posteriors on the lattice with optional spans: the numpy yardstick (tests/span_posterior_reference.py) against
brute-force enumeration of all paths, its identities, the spectrum of the device test's inputs, and the host face of
la_alignment_posteriors_spans (declared, exported, argument checks answered before any device call)."""
import ctypes
import os
import re

import numpy as np
import pytest

import posterior_reference as pr
import span_posterior_reference as spr
from conftest import ROOT

ENUM = [  # (T, labels, spans, what)
    (6, [3, 7, 5], [(1, 2), (0, 3)], "nested spans, one ending at L, one starting at 0"),
    (6, [3, 7, 5], [(0, 1), (0, 3)], "two spans sharing a start"),
    (7, [2, 9, 9], [(1, 3)], "a repeated label inside a span that ends at L"),
    (6, [4, 4, 6], [(0, 1), (1, 3)], "adjacent spans, repeated label at the seam"),
    (7, [5, 6, 5], [(1, 2)], "J-1 arc into the odd target barred by equal labels"),
    (5, [8, 3], [(0, 2)], "everything optional"),
    (6, [3, 7, 5], [(0, 2), (1, 3)], "overlapping spans"),
]


def _skip_from(L, spans):
    sf = [-1] * (L + 1)
    for a, n in spans:
        sf[n] = a
    return sf


@pytest.mark.parametrize("penalty", [0.0, 0.7])
@pytest.mark.parametrize("T,labels,spans,what", ENUM, ids=[c[3].replace(" ", "_").replace(",", "") for c in ENUM])
def test_reference_equals_brute_force_enumeration(T, labels, spans, what, penalty):
    """Pins the yardstick: gamma, log_z, present and span_skip of the float64 forward-backward equal the sums over ALL paths within
    1e-12, and the coverage identity holds for every label."""
    rs = np.random.RandomState(200 + T + len(spans))
    L = len(labels)
    em = pr.fix_repeats((-rs.rand(T, L + 1) * 3).astype(np.float32), labels)
    sf = _skip_from(L, spans)
    gamma, entry, exit_, present, span_skip, log_z = spr.posteriors(em, labels, sf, penalty)
    gamma_b, log_z_b, present_b, skip_b = spr.brute(em, labels, sf, penalty)
    worst = {"gamma": np.abs(gamma - gamma_b).max(), "log_z": abs(log_z - log_z_b), "present": np.abs(present - present_b).max(),
             "span_skip": np.abs(span_skip - skip_b).max(), "coverage": np.abs(spr.coverage(present, span_skip, sf) - 1).max(),
             "rowsum": np.abs(gamma.sum(1) - 1).max(), "exit": np.abs(exit_.sum(0) - present).max()}
    print(what, penalty, "span_skip", np.round(span_skip, 4), "present", np.round(present, 4), worst)
    for k, v in worst.items():
        assert v <= 1e-12, (what, k, v)
    assert span_skip.max() > 1e-3                                      # the jumps carry mass in these cases
    assert not span_skip[[n for n in range(L + 1) if sf[n] < 0]].any()  # 0 where no span ends
    # a label occupies frame t iff it was entered at or before t and left at or after t
    occ_from_edges = np.cumsum(entry, 0) - np.cumsum(exit_, 0) + exit_
    assert np.abs(occ_from_edges - gamma[:, 1::2]).max() <= 1e-12


def test_coverage_identity_on_random_spans():
    """present[n] + the mass of every span over n = 1 for every label, with random (nested, overlapping, start-sharing) spans."""
    for seed in range(6):
        rs = np.random.RandomState(seed)
        T, L = 30 + 5 * seed, 9 + seed
        labels = [int(v) for v in rs.randint(1, 6, size=L)]
        em = pr.fix_repeats((-rs.rand(T, L + 1) * 4 - (seed % 2) * 1.5 * (np.arange(L + 1) > 0)).astype(np.float32), labels)
        sf = [-1] * (L + 1)
        for n in range(1, L + 1):
            if rs.rand() < 0.4:
                sf[n] = int(rs.randint(max(0, n - 5), n))
        gamma, entry, exit_, present, span_skip, log_z = spr.posteriors(em, labels, sf, 0.5 * (seed % 3))
        assert np.abs(spr.coverage(present, span_skip, sf) - 1).max() <= 1e-12
        assert np.abs(gamma.sum(1) - 1).max() <= 1e-12
        assert (present <= 1 + 1e-12).all() and (span_skip >= 0).all()


def test_without_spans_equals_the_plain_yardstick():
    for T, L, seed in ((40, 7, 1), (12, 5, 2)):
        em, labels = pr.make_inputs(T, L, 3.0, seed)
        want = pr.posteriors(em, labels)
        for pen in (0.0, 0.7):
            gamma, entry, exit_, present, span_skip, log_z = spr.posteriors(em, labels, [-1] * (L + 1), pen)
            for got, ref in zip((gamma, entry, exit_, log_z), want):
                assert np.abs(got - ref).max() <= 1e-12
            assert np.abs(present - 1).max() <= 1e-12 and not span_skip.any()
    labels = [3, 5, 5, 7]                       # infeasible: zero mass, as the plain yardstick
    em = pr.fix_repeats((-np.random.RandomState(0).rand(4, 5) * 3).astype(np.float32), labels)
    res = spr.posteriors(em, labels, [-1] * 5)
    assert np.isneginf(res[5]) and not any(np.asarray(v).any() for v in res[:5])


def test_a_large_penalty_closes_the_jumps():
    em, labels, sf = spr.make_inputs(40, [2, 2], {1}, 3.0, 7, 6.0)
    gamma, entry, exit_, present, span_skip, log_z = spr.posteriors(em, labels, sf, 1e4)
    assert (span_skip == 0).all()
    assert abs(log_z - pr.posteriors(em, labels)[3]) <= 1e-12


def test_the_device_tests_inputs_cover_certain_impossible_and_undecided_spans():
    """Keeps tests/test_gpu_span_posteriors.py from being vacuous: over its generator cases and penalties the yardstick's span_skip
    values of the declared spans hold at least one above 0.99, one below 0.01 and one in [0.05, 0.95]."""
    values = []
    for case in spr.GENERATOR_CASES:
        em, labels, sf = spr.make_inputs(*case)
        for pen in spr.PENALTIES:
            span_skip = spr.posteriors(em, labels, sf, pen)[4]
            got = [float(span_skip[n]) for _, n in spr.spans_of(sf)]
            print(case, "penalty", pen, "span_skip", np.round(got, 4))
            values += got
    v = np.asarray(values)
    assert (v > 0.99).any() and (v < 0.01).any() and ((v >= 0.05) & (v <= 0.95)).any()
    # the figures of the feature's description
    em, labels, sf = spr.make_inputs(150, [3] * 5, {2}, 3.0, 3, 0.3)
    assert abs(spr.posteriors(em, labels, sf, 0.0)[4][9] - 0.52) < 0.01 and abs(spr.posteriors(em, labels, sf, 1.0)[4][9] - 0.29) < 0.01
    em, labels, sf = spr.make_inputs(150, [3] * 5, {2}, 3.0, 3, 6.0)
    assert spr.posteriors(em, labels, sf, 0.0)[4][9] > 0.9999
    em, labels, sf = spr.make_inputs(40, [2, 2], {1}, 3.0, 7, 6.0)
    assert abs(spr.posteriors(em, labels, sf, 0.0)[4][4] - 0.996) < 0.002
    em, labels, sf = spr.make_inputs(40, [2, 2], {0}, 3.0, 7, 0.3)
    assert abs(spr.posteriors(em, labels, sf, 0.0)[4][2] - 0.004) < 0.002


def test_span_posteriors_entry_points_are_declared_exported_and_check_arguments_on_the_host():
    from lyricalignment_amd import _lib
    text = open(os.path.join(ROOT, "include", "lyricalign.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("la_alignment_posteriors_spans_workspace_bytes", "la_alignment_posteriors_spans"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in lyricalign.h"
        assert name in _lib.SYMBOLS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} not exported"
    L = _lib.lib()
    need = ctypes.c_size_t(0)
    plain = ctypes.c_size_t(0)
    for shape in ((32, 1500, 26), (1, 9000, 238), (1, 600, 511)):       # the alpha workspace keeps its size formula
        assert L.la_alignment_posteriors_spans_workspace_bytes(*shape, ctypes.byref(need)) == _lib.LA_OK
        assert L.la_alignment_posteriors_workspace_bytes(*shape, ctypes.byref(plain)) == _lib.LA_OK
        assert need.value == plain.value > 0
    assert L.la_alignment_posteriors_spans_workspace_bytes(32, 1500, 26, ctypes.byref(need)) == _lib.LA_OK and need.value == 32 * 1500 * 64 * 8
    assert L.la_alignment_posteriors_spans_workspace_bytes(1, 600, 512, ctypes.byref(need)) == _lib.LA_EUNSUPPORTED and "511" in _lib.last_error()
    assert L.la_alignment_posteriors_spans_workspace_bytes(1, 600, 26, None) == _lib.LA_EINVAL

    P = 16                                      # a non-null, aligned stand-in pointer: every call below is refused before any device call
    big = 1 << 40

    def call(em=P, labels=P, n_labels=P, n_frames=P, batch=2, T=100, Lmax=26, onset=P, offset=P, out_stride=26, w=2, skip=P, skip_stride=27,
             pen=0.0, occ=P, onp=P, offp=P, pres=P, skp=P, log_z=P, status=P, gamma=0, gbs=0, grs=0, ws=P, ws_bytes=big, em_rs=27, labels_stride=26):
        return L.la_alignment_posteriors_spans(em, T * em_rs, em_rs, labels, labels_stride, n_labels, n_frames, batch, T, Lmax, onset, offset,
                                               out_stride, w, skip, skip_stride, pen, occ, onp, offp, pres, skp, log_z, status, gamma, gbs, grs,
                                               ws, ws_bytes, 0)

    for null in ("occ", "onp", "offp", "pres", "skp", "log_z", "status", "em", "onset", "offset", "skip"):
        assert call(**{null: 0}) == _lib.LA_EINVAL, null
        assert "null" in _lib.last_error()
    assert call(w=-1) == _lib.LA_EINVAL and "boundary_window" in _lib.last_error()
    assert call(pen=-0.5) == _lib.LA_EINVAL and "skip_penalty" in _lib.last_error()
    assert call(pen=float("nan")) == _lib.LA_EINVAL and "skip_penalty" in _lib.last_error()
    assert call(skip_stride=26) == _lib.LA_EINVAL and "strides" in _lib.last_error()
    assert call(out_stride=25) == _lib.LA_EINVAL and "strides" in _lib.last_error()
    assert call(em_rs=26) == _lib.LA_EINVAL
    assert call(gamma=P, gbs=100 * 53, grs=52) == _lib.LA_EINVAL and "gamma" in _lib.last_error()
    assert call(Lmax=512, out_stride=512, em_rs=513, labels_stride=512, skip_stride=513) == _lib.LA_EUNSUPPORTED and "511" in _lib.last_error()
    assert call(ws_bytes=2 * 100 * 64 * 8 - 1) == _lib.LA_EINVAL and "workspace too small" in _lib.last_error()
    assert call(ws=0) == _lib.LA_EINVAL
    assert call(batch=0) == _lib.LA_OK          # nothing to do, nothing enqueued
