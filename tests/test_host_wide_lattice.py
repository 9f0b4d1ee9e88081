"""Whole-song lattices without a GPU (la_viterbi_lattice_batch, ops.viterbi_lattice_batch, the route of utils.alignment.run_lattice beyond
511 labels): the workspace query's values, the argument errors answered on the host before any device call, the calls run_lattice makes
with the ops.* lattice functions replaced by recorders, and the yardstick of tests/test_gpu_wide_lattice.py -- windows_reference with
rows=True, which has no label limit -- against the oracle beyond 511 labels."""
import ctypes

import numpy as np
import pytest
import torch

import windows_reference as wr

DP = ("viterbi_batch", "viterbi_spans_batch", "viterbi_windows_batch", "viterbi_lattice_batch")
POST = ("alignment_posteriors", "alignment_posteriors_spans", "alignment_posteriors_windows")


# ------------------------------------------------------------------------------------------------ 1. the workspace query
def test_workspace_query_values_and_the_limits_of_the_existing_queries():
    from lyricalignment_amd import _lib
    L = _lib.lib()
    need, other = ctypes.c_size_t(1), ctypes.c_size_t(2)
    f = L.la_viterbi_lattice_workspace_bytes
    for shape, want in (((1, 100, 512), 76800), ((1, 100, 600), 76800), ((2, 100, 4095), 614400)):
        assert f(*shape, ctypes.byref(need)) == _lib.LA_OK and need.value == want, shape
    # above 511 labels: batch * max_frames * R * 16 * 3 * 8 with R = 2, 4, 8 states per thread
    for labels, R in ((512, 2), (1023, 2), (1024, 4), (2047, 4), (2048, 8), (4095, 8)):
        assert f(3, 70, labels, ctypes.byref(need)) == _lib.LA_OK and need.value == 3 * 70 * R * 16 * 3 * 8, labels
    assert f(1, 100, 4096, ctypes.byref(need)) == _lib.LA_EUNSUPPORTED and "4095" in _lib.last_error()
    assert f(1, 100, 26, None) == _lib.LA_EINVAL
    for shape in ((32, 1500, 26), (1, 600, 511), (1, 40, 511)):                                  # the span planner's answers
        assert f(*shape, ctypes.byref(need)) == _lib.LA_OK
        assert L.la_viterbi_spans_workspace_bytes(*shape, ctypes.byref(other)) == _lib.LA_OK and need.value == other.value, shape
    for g in (L.la_viterbi_spans_workspace_bytes, L.la_viterbi_windows_workspace_bytes):          # the existing queries still refuse 512
        assert g(1, 100, 512, ctypes.byref(other)) == _lib.LA_EUNSUPPORTED and "511" in _lib.last_error()
    assert L.la_version() == 2


# ------------------------------------------------------------------------------------------------ 2. argument errors, on the host
def test_lattice_entry_checks_its_arguments_on_the_host():
    from lyricalignment_amd import _lib
    L = _lib.lib()
    P = 16                                      # a non-null, aligned stand-in pointer: every call below is refused before any device call
    big = 1 << 40

    def call(em=P, labels=P, n_labels=P, n_frames=P, batch=2, T=100, Lmax=600, onset=P, offset=P, out_stride=None, score=P, status=P,
             skip_from=P, skip_stride=None, penalty=0.0, win_lo=P, win_hi=P, win_stride=None, ws=P, ws_bytes=big, em_rs=None,
             labels_stride=None):
        out_stride = Lmax if out_stride is None else out_stride
        skip_stride = Lmax + 1 if skip_stride is None else skip_stride
        win_stride = 2 * Lmax + 1 if win_stride is None else win_stride
        em_rs = Lmax + 1 if em_rs is None else em_rs
        labels_stride = Lmax if labels_stride is None else labels_stride
        return L.la_viterbi_lattice_batch(em, T * em_rs, em_rs, labels, labels_stride, n_labels, n_frames, batch, T, Lmax, onset, offset,
                                          out_stride, score, status, skip_from, skip_stride, penalty, win_lo, win_hi, win_stride,
                                          ws, ws_bytes, 0)

    for Lmax in (26, 600):                       # below and above the limit of the lane-per-state entries: the same answers
        for null in ("em", "labels", "n_labels", "n_frames", "onset", "offset", "score", "status"):
            assert call(Lmax=Lmax, **{null: 0}) == _lib.LA_EINVAL, null
            assert "null" in _lib.last_error() and "viterbi_lattice_batch" in _lib.last_error()
        for one in ("win_lo", "win_hi"):         # one window pointer without the other
            assert call(Lmax=Lmax, **{one: 0}) == _lib.LA_EINVAL, one
            assert "win_lo and win_hi" in _lib.last_error()
        assert call(Lmax=Lmax, win_stride=2 * Lmax) == _lib.LA_EINVAL and "strides" in _lib.last_error()
        assert call(Lmax=Lmax, skip_stride=Lmax) == _lib.LA_EINVAL and "strides" in _lib.last_error()
        assert call(Lmax=Lmax, out_stride=Lmax - 1) == _lib.LA_EINVAL
        assert call(Lmax=Lmax, em_rs=Lmax) == _lib.LA_EINVAL
        assert call(Lmax=Lmax, labels_stride=Lmax - 1) == _lib.LA_EINVAL
        for pen in (-0.5, float("nan")):
            assert call(Lmax=Lmax, penalty=pen) == _lib.LA_EINVAL and "skip_penalty" in _lib.last_error()
            assert call(Lmax=Lmax, penalty=pen, skip_from=0, win_lo=0, win_hi=0) == _lib.LA_EINVAL
        assert call(Lmax=Lmax, T=0) == _lib.LA_EINVAL
        assert call(Lmax=Lmax, batch=0) == _lib.LA_OK                    # nothing to do, nothing enqueued
    # the strides of a pointer that is absent are not looked at (the refusal below is the workspace's, the last check)
    assert call(skip_from=0, skip_stride=0, ws=0) == _lib.LA_EINVAL and "workspace" in _lib.last_error()
    assert call(win_lo=0, win_hi=0, win_stride=0, ws=0) == _lib.LA_EINVAL and "workspace" in _lib.last_error()
    assert call(ws_bytes=2 * 100 * 2 * 16 * 3 * 8 - 1) == _lib.LA_EINVAL and "workspace too small" in _lib.last_error()
    assert call(ws=P + 4) == _lib.LA_EINVAL and "aligned" in _lib.last_error()
    assert call(Lmax=4096) == _lib.LA_EUNSUPPORTED and "4095" in _lib.last_error()
    assert call(Lmax=4096, skip_from=0, win_lo=0, win_hi=0) == _lib.LA_EUNSUPPORTED and "4095" in _lib.last_error()


# ------------------------------------------------------------------------------------------------ 3. run_lattice with recorders
@pytest.fixture
def calls(monkeypatch):
    from lyricalignment_amd import ops
    log = []

    def recorder(name):
        def call(*args, **kw):
            assert not kw
            log.append((name, args))
            B, Lmax = args[1].shape
            tag = float(len(log))
            if name in DP:
                return tuple(torch.full((B, Lmax), tag + i / 8) for i in range(2)) + tuple(torch.full((B,), tag + i / 8) for i in (2, 3))
            out = tuple(torch.full((B, Lmax), tag + i / 8) for i in range(3)) + (torch.full((B,), tag + 0.375), torch.full((B,), tag + 0.5))
            return out if name == "alignment_posteriors" else out + (torch.full((B, Lmax), tag + 0.625), torch.full((B, Lmax + 1), tag + 0.75))
        return call
    for name in DP + POST:
        monkeypatch.setattr(ops, name, recorder(name))
    return log


def _inputs(Lmax, B=2, T=6):
    em, lab = torch.zeros((B, T, Lmax + 1)), torch.ones((B, Lmax), dtype=torch.int32)
    n_lab, nf = torch.full((B,), Lmax, dtype=torch.int32), torch.full((B,), T, dtype=torch.int32)
    skip = torch.full((B, Lmax + 1), -1, dtype=torch.int32)
    skip[0, 2] = 0
    win = (torch.zeros((B, 2 * Lmax + 1), dtype=torch.int32), torch.full((B, 2 * Lmax + 1), T, dtype=torch.int32))
    return em, lab, n_lab, nf, skip, win


@pytest.mark.parametrize("has_spans,has_win", [(True, False), (False, True), (True, True)])
def test_run_lattice_beyond_511_labels_calls_the_general_entry_once(calls, has_spans, has_win):
    from lyricalignment_amd.utils import alignment as ua
    em, lab, n_lab, nf, skip, win = _inputs(512)
    given = tuple(torch.full(s, 9.0) for s in ((2, 512), (2, 512), (2,), (2,)))
    for dp in (None, given):                                                 # a DP result that exists is the plain lattice's only
        del calls[:]
        r = ua.run_lattice(em, lab, n_lab, nf, skip if has_spans else None, win if has_win else None, 1.5, None, 3, dp=dp)
        assert [name for name, _ in calls] == ["viterbi_lattice_batch"]
        args = calls[0][1]
        assert all(a is b for a, b in zip(args[:4], (em, lab, n_lab, nf))) and len(args) == 8
        assert torch.equal(args[4], skip) if has_spans else args[4] is None
        assert args[5] == 1.5
        if has_win:
            assert torch.equal(args[6], win[0]) and torch.equal(args[7], win[1])
        else:
            assert args[6] is None and args[7] is None
        assert [float(t.flatten()[0]) for t in r[:4]] == [1.0, 1.125, 1.25, 1.375] and all(v is None for v in r[4:])


def test_run_lattice_beyond_511_labels_plain_and_at_511_labels_as_before(calls):
    from lyricalignment_amd.utils import alignment as ua
    em, lab, n_lab, nf, skip, win = _inputs(512)
    ua.run_lattice(em, lab, n_lab, nf)
    assert [name for name, _ in calls] == ["viterbi_batch"] and len(calls[0][1]) == 4
    del calls[:]
    given = tuple(torch.full(s, 9.0) for s in ((2, 512), (2, 512), (2,), (2,)))
    r = ua.run_lattice(em, lab, n_lab, nf, dp=given)                          # the fused head's result is taken as it is
    assert calls == [] and all(a is b for a, b in zip(r[:4], given))
    em, lab, n_lab, nf, skip, win = _inputs(511)
    for s, w, want in ((None, None, "viterbi_batch"), (skip, None, "viterbi_spans_batch"), (None, win, "viterbi_windows_batch"),
                       (skip, win, "viterbi_windows_batch")):
        del calls[:]
        ua.run_lattice(em, lab, n_lab, nf, s, w, 1.5)
        assert [name for name, _ in calls] == [want]
    for conf, s, w, want in (("plain", None, None, ["viterbi_batch", "alignment_posteriors"]),
                             ("span", skip, None, ["viterbi_spans_batch", "alignment_posteriors_spans"]),
                             ("anchored", skip, win, ["viterbi_windows_batch", "alignment_posteriors_windows", "alignment_posteriors_spans"])):
        del calls[:]
        ua.run_lattice(em, lab, n_lab, nf, s, w, 1.5, conf, 2)
        assert [name for name, _ in calls] == want


@pytest.mark.parametrize("conf", ["plain", "span", "anchored"])
def test_any_confidence_beyond_511_labels_is_refused_before_a_call(calls, conf):
    from lyricalignment_amd.utils import alignment as ua
    em, lab, n_lab, nf, skip, win = _inputs(512)
    for s, w in ((None, None), (skip, None), (None, win), (skip, win)):
        with pytest.raises(NotImplementedError, match="511"):
            ua.run_lattice(em, lab, n_lab, nf, s, w, 1.5, conf, 2)
    assert calls == []


# ------------------------------------------------------------------------------------------------ 4. the yardstick beyond 511 labels
def test_the_yardstick_equals_the_oracle_beyond_511_labels():
    """windows_reference.viterbi_windows(rows=True) at (T, L) = (700, 600) with open windows and no span against the oracle's
    align_frames_compact: frames, the score's bits and the status."""
    from oracle.alignment_oracle import align_frames_compact
    from test_gpu_windows import _emissions, _labels
    T, L = 700, 600
    lab = _labels(7 * T + L, L)
    em = _emissions(100, T, lab, 0.0)
    on, off, score, status, path = wr.viterbi_windows(em, lab, *wr.open_windows(L, T), None, 0.0, rows=True)
    assert status == wr.LA_OK and len(path) == T
    rc, want_on, want_off, want_score = align_frames_compact(em, np.asarray(lab))
    assert rc == status == wr.LA_OK
    assert want_on.tolist() == on and want_off.tolist() == off
    assert np.float64(want_score).tobytes() == np.float64(score).tobytes()
