"""CPU-only checks of the alignment posteriors: the numpy yardstick (tests/posterior_reference.py) against brute-force
enumeration of all paths, and the host face of la_alignment_posteriors (declared, exported, argument checks answered
before any device call)."""
import ctypes
import os
import re

import numpy as np
import pytest

import posterior_reference as pr
from conftest import ROOT


@pytest.mark.parametrize("T,labels", [(5, [3, 7]), (6, [3, 3, 5]), (7, [2, 9, 9]), (4, [5])], ids=lambda v: str(v).replace(" ", ""))
def test_reference_equals_brute_force_enumeration(T, labels):
    """Pins the yardstick: gamma and log_z of the float64 forward-backward equal the sum over ALL paths within 1e-12
    (measured 1e-15); gamma rows, entry columns and exit columns each sum to 1."""
    rs = np.random.RandomState(100 + T)
    em = pr.fix_repeats((-rs.rand(T, len(labels) + 1) * 4).astype(np.float32), labels)
    gamma, entry, exit_, log_z = pr.posteriors(em, labels)
    gamma_b, log_z_b = pr.brute(em, labels)
    print("max |gamma - brute|", np.abs(gamma - gamma_b).max(), "|log_z - brute|", abs(log_z - log_z_b))
    assert np.abs(gamma - gamma_b).max() <= 1e-12
    assert abs(log_z - log_z_b) <= 1e-12
    assert np.abs(gamma.sum(1) - 1).max() <= 1e-12
    assert np.abs(entry.sum(0) - 1).max() <= 1e-12
    assert np.abs(exit_.sum(0) - 1).max() <= 1e-12
    # a label occupies frame t iff it was entered at or before t and left at or after t
    occ_from_edges = np.cumsum(entry, 0) - np.cumsum(exit_, 0) + exit_
    assert np.abs(occ_from_edges - gamma[:, 1::2]).max() <= 1e-12
    # the DP's path is one of the enumerated paths: its posterior is at most 1
    on, off, score = pr.viterbi(em, labels)
    assert score - log_z <= 1e-12 and min(on) >= 0


def test_reference_reports_no_path_as_zero_mass():
    labels = [3, 5, 5, 7]                       # the repeat needs a silence frame in between: 5 frames, not 4
    em = pr.fix_repeats((-np.random.RandomState(0).rand(4, 5) * 3).astype(np.float32), labels)
    gamma, entry, exit_, log_z = pr.posteriors(em, labels)
    assert np.isneginf(log_z) and not gamma.any() and not entry.any() and not exit_.any()


def test_posteriors_entry_points_are_declared_exported_and_check_arguments_on_the_host():
    from lyricalignment_amd import _lib
    text = open(os.path.join(ROOT, "include", "lyricalign.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("la_alignment_posteriors_workspace_bytes", "la_alignment_posteriors"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in lyricalign.h"
        assert name in _lib.SYMBOLS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} not exported"
    L = _lib.lib()
    assert L.la_version() == 2
    need = ctypes.c_size_t(0)
    # alpha rows [batch][max_frames][S_pad] float64, S_pad = 64 * (power-of-two wave count holding 2 max_labels + 1 states)
    assert L.la_alignment_posteriors_workspace_bytes(32, 1500, 26, ctypes.byref(need)) == _lib.LA_OK and need.value == 32 * 1500 * 64 * 8
    assert L.la_alignment_posteriors_workspace_bytes(1, 9000, 238, ctypes.byref(need)) == _lib.LA_OK and need.value == 9000 * 512 * 8
    assert L.la_alignment_posteriors_workspace_bytes(1, 600, 511, ctypes.byref(need)) == _lib.LA_OK and need.value == 600 * 1024 * 8
    assert L.la_alignment_posteriors_workspace_bytes(1, 600, 512, ctypes.byref(need)) == _lib.LA_EUNSUPPORTED and "511" in _lib.last_error()
    assert L.la_alignment_posteriors_workspace_bytes(1, 600, 26, None) == _lib.LA_EINVAL

    P = 16                                      # a non-null, aligned stand-in pointer: every call below is refused before any device call
    big = 1 << 40

    def call(em=P, labels=P, n_labels=P, n_frames=P, batch=2, T=100, Lmax=26, onset=P, offset=P, out_stride=26, w=2, occ=P, onp=P, offp=P,
             log_z=P, status=P, gamma=0, gbs=0, grs=0, ws=P, ws_bytes=big, em_rs=27, labels_stride=26):
        return L.la_alignment_posteriors(em, T * em_rs, em_rs, labels, labels_stride, n_labels, n_frames, batch, T, Lmax, onset, offset,
                                         out_stride, w, occ, onp, offp, log_z, status, gamma, gbs, grs, ws, ws_bytes, 0)

    for null in ("occ", "onp", "offp", "log_z", "status", "em", "onset", "offset"):
        assert call(**{null: 0}) == _lib.LA_EINVAL, null
        assert "null" in _lib.last_error()
    assert call(w=-1) == _lib.LA_EINVAL and "boundary_window" in _lib.last_error()
    assert call(out_stride=25) == _lib.LA_EINVAL and "strides" in _lib.last_error()
    assert call(em_rs=26) == _lib.LA_EINVAL
    assert call(gamma=P, gbs=100 * 53, grs=52) == _lib.LA_EINVAL and "gamma" in _lib.last_error()
    assert call(Lmax=512, out_stride=512, em_rs=513, labels_stride=512) == _lib.LA_EUNSUPPORTED and "511" in _lib.last_error()
    assert call(ws_bytes=2 * 100 * 64 * 8 - 1) == _lib.LA_EINVAL and "workspace too small" in _lib.last_error()
    assert call(ws=0) == _lib.LA_EINVAL
    assert call(batch=0) == _lib.LA_OK          # nothing to do, nothing enqueued
    with pytest.raises(NotImplementedError):
        _lib.check(L.la_alignment_posteriors_workspace_bytes(1, 600, 512, ctypes.byref(need)), "x")
