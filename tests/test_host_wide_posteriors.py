"""Whole-song posteriors without a GPU (la_alignment_posteriors_lattice, ops.alignment_posteriors_lattice, run_lattice(confidence="sheet"),
AlignModel.align(return_sheet_confidence=True), harness.align_song): the workspace query's values, the argument errors answered on the host
before any device call under the entry's own name, the calls run_lattice makes with the ops.* lattice functions replaced by recorders, the
surface's refusals, and the spans and anchors align_song hands to the model for the three forms of a sheet."""
import ctypes

import pytest
import torch

DP = ("viterbi_batch", "viterbi_spans_batch", "viterbi_windows_batch", "viterbi_lattice_batch")
POST = ("alignment_posteriors", "alignment_posteriors_spans", "alignment_posteriors_windows", "alignment_posteriors_lattice")
WHO = "alignment_posteriors_lattice"


# ------------------------------------------------------------------------------------------------ H1. the workspace query
def test_workspace_query_values():
    from lyricalignment_amd import _lib
    L = _lib.lib()
    need, other = ctypes.c_size_t(1), ctypes.c_size_t(2)
    f = L.la_alignment_posteriors_lattice_workspace_bytes
    for shape in ((32, 1500, 26), (1, 600, 511), (3, 40, 511), (2, 90, 31)):                      # the existing queries' answers, each face
        assert f(*shape, ctypes.byref(need)) == _lib.LA_OK
        for g in (L.la_alignment_posteriors_workspace_bytes, L.la_alignment_posteriors_spans_workspace_bytes,
                  L.la_alignment_posteriors_windows_workspace_bytes):
            assert g(*shape, ctypes.byref(other)) == _lib.LA_OK and need.value == other.value, shape
    for labels, R in ((512, 2), (1023, 2), (1024, 4), (2047, 4), (2048, 8), (4095, 8)):
        for batch, frames in ((1, 100), (3, 70)):
            assert f(batch, frames, labels, ctypes.byref(need)) == _lib.LA_OK
            rows = batch * frames * 1024 * R * 8
            # the alpha rows, plus per clip and state 20 bytes of sparse sums and 8 bytes of jump arcs
            assert rows <= need.value == rows + batch * 1024 * R * 28, (labels, batch, frames)
    # a four-minute song: 197 MB at 800 labels, 786 MB of alpha rows (and 0.2 MB beside them) at 2500 .. 4095
    assert f(1, 12000, 800, ctypes.byref(need)) == _lib.LA_OK and 196.6e6 <= need.value < 196.7e6
    for labels in (2500, 4095):
        assert f(1, 12000, labels, ctypes.byref(need)) == _lib.LA_OK and 786.4e6 <= need.value < 786.7e6
    assert f(1, 100, 4096, ctypes.byref(need)) == _lib.LA_EUNSUPPORTED and "4095" in _lib.last_error() and WHO in _lib.last_error()
    assert f(1, 100, 26, None) == _lib.LA_EINVAL and WHO in _lib.last_error()
    assert f(1, 0, 26, ctypes.byref(need)) == _lib.LA_EINVAL
    for g in (L.la_alignment_posteriors_workspace_bytes, L.la_alignment_posteriors_spans_workspace_bytes,
              L.la_alignment_posteriors_windows_workspace_bytes):                                 # the existing queries still refuse 512
        assert g(1, 100, 512, ctypes.byref(other)) == _lib.LA_EUNSUPPORTED and "511" in _lib.last_error()


# ------------------------------------------------------------------------------------------------ H2. argument errors, on the host
def test_lattice_posteriors_entry_checks_its_arguments_on_the_host():
    from lyricalignment_amd import _lib
    L = _lib.lib()
    P = 16                                      # a non-null, aligned stand-in pointer: every call below is refused before any device call
    big = 1 << 42

    def call(em=P, labels=P, n_labels=P, n_frames=P, batch=2, T=100, Lmax=600, onset=P, offset=P, out_stride=None, window=2, skip_from=P,
             skip_stride=None, penalty=0.0, win_lo=P, win_hi=P, win_stride=None, occ=P, onp=P, offp=P, pres=P, skp=P, log_z=P, status=P,
             gamma=0, gamma_bs=0, gamma_rs=0, ws=P, ws_bytes=big, em_rs=None, labels_stride=None):
        out_stride = Lmax if out_stride is None else out_stride
        skip_stride = Lmax + 1 if skip_stride is None else skip_stride
        win_stride = 2 * Lmax + 1 if win_stride is None else win_stride
        em_rs = Lmax + 1 if em_rs is None else em_rs
        labels_stride = Lmax if labels_stride is None else labels_stride
        return L.la_alignment_posteriors_lattice(em, T * em_rs, em_rs, labels, labels_stride, n_labels, n_frames, batch, T, Lmax, onset, offset,
                                                 out_stride, window, skip_from, skip_stride, penalty, win_lo, win_hi, win_stride, occ, onp,
                                                 offp, pres, skp, log_z, status, gamma, gamma_bs, gamma_rs, ws, ws_bytes, 0)

    def refused(rc, *words):
        msg = _lib.last_error()
        return rc == _lib.LA_EINVAL and WHO in msg and all(w in msg for w in words)

    for Lmax in (26, 600):                       # below and above the limit of the lane-per-state entries: the same answers
        for null in ("em", "labels", "n_labels", "n_frames", "onset", "offset", "occ", "onp", "offp", "pres", "skp", "log_z", "status"):
            assert refused(call(Lmax=Lmax, **{null: 0}), "null"), null
        for one in ("win_lo", "win_hi"):         # one window pointer without the other
            assert refused(call(Lmax=Lmax, **{one: 0}), "win_lo and win_hi"), one
        assert refused(call(Lmax=Lmax, win_stride=2 * Lmax), "strides")
        assert refused(call(Lmax=Lmax, skip_stride=Lmax), "strides")
        assert refused(call(Lmax=Lmax, skip_stride=Lmax, skip_from=0), "strides")       # still the row pitch of span_skip_prob
        assert refused(call(Lmax=Lmax, out_stride=Lmax - 1), "strides")
        assert refused(call(Lmax=Lmax, em_rs=Lmax), "strides")
        assert refused(call(Lmax=Lmax, labels_stride=Lmax - 1), "strides")
        for pen in (-0.5, float("nan")):
            assert refused(call(Lmax=Lmax, penalty=pen), "skip_penalty")
            assert refused(call(Lmax=Lmax, penalty=pen, skip_from=0, win_lo=0, win_hi=0), "skip_penalty")
        assert refused(call(Lmax=Lmax, T=0), "sizes")
        assert refused(call(Lmax=Lmax, batch=-1), "sizes")
        assert refused(call(Lmax=Lmax, window=-1), "boundary_window")
        assert refused(call(Lmax=Lmax, gamma=P, gamma_rs=2 * Lmax, gamma_bs=big), "gamma strides")
        assert refused(call(Lmax=Lmax, gamma=P, gamma_rs=2 * Lmax + 1, gamma_bs=100 * (2 * Lmax + 1) - 1), "gamma strides")
        assert refused(call(Lmax=Lmax, ws=0), "workspace")
        assert refused(call(Lmax=Lmax, ws=P + 4), "aligned")
        assert call(Lmax=Lmax, batch=0) == _lib.LA_OK                    # nothing to do, nothing enqueued
    # the window stride of absent windows is not looked at (the refusal below is the workspace's, the last check)
    assert refused(call(win_lo=0, win_hi=0, win_stride=0, ws=0), "workspace")
    assert refused(call(ws_bytes=2 * 100 * 2048 * 8 + 2 * 2048 * 28 - 1), "workspace too small")
    assert refused(call(Lmax=26, ws_bytes=2 * 100 * 64 * 8 - 1), "workspace too small")
    for more in ({}, dict(skip_from=0, win_lo=0, win_hi=0)):
        assert call(Lmax=4096, **more) == _lib.LA_EUNSUPPORTED and "4095" in _lib.last_error() and WHO in _lib.last_error()


# ------------------------------------------------------------------------------------------------ H3. run_lattice with recorders
@pytest.fixture
def calls(monkeypatch):
    from lyricalignment_amd import ops
    log = []

    def recorder(name):
        def call(*args, **kw):
            log.append((name, args, kw))
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


def _lattice_call_args(entry):
    """(name, args, kw) of a recorded ops.alignment_posteriors_lattice call -> skip_from, skip_penalty, win_lo, win_hi, boundary_window."""
    names = ("skip_from", "skip_penalty", "win_lo", "win_hi", "boundary_window", "want_gamma")
    given = dict(zip(names, entry[1][6:]))
    given.update(entry[2])
    return tuple(given.get(k, d) for k, d in zip(names[:5], (None, 0.0, None, None, 2)))


@pytest.mark.parametrize("Lmax", [511, 512])
@pytest.mark.parametrize("has_spans,has_win", [(False, False), (True, False), (False, True), (True, True)])
def test_run_lattice_sheet_confidence_routing(calls, Lmax, has_spans, has_win):
    from lyricalignment_amd.utils import alignment as ua
    em, lab, n_lab, nf, skip, win = _inputs(Lmax)
    r = ua.run_lattice(em, lab, n_lab, nf, skip if has_spans else None, win if has_win else None, 1.5, "sheet", 3)
    if Lmax > 511:
        dp = "viterbi_lattice_batch" if has_spans or has_win else "viterbi_batch"
    else:
        dp = "viterbi_windows_batch" if has_win else "viterbi_spans_batch" if has_spans else "viterbi_batch"
    assert [name for name, _, _ in calls] == [dp] + ["alignment_posteriors_lattice"] * (2 if has_win else 1)   # today's DP, then the sweep(s)
    for entry in calls[1:]:
        args = entry[1]
        assert all(a is b for a, b in zip(args[:4], (em, lab, n_lab, nf)))
        assert float(args[4].flatten()[0]) == 1.0 and float(args[5].flatten()[0]) == 1.125          # the DP's onset / offset
    s, pen, lo, hi, bw = _lattice_call_args(calls[1])
    assert (torch.equal(s, skip) if has_spans else s is None) and pen == 1.5 and bw == 3
    assert (torch.equal(lo, win[0]) and torch.equal(hi, win[1])) if has_win else (lo is None and hi is None)
    if has_win:                                                                                    # the second call: the same lattice without windows
        s, pen, lo, hi, bw = _lattice_call_args(calls[2])
        assert (torch.equal(s, skip) if has_spans else s is None) and pen == 1.5 and lo is None and hi is None
    # filled exactly as "anchored": the DP's four, the sweep's occupancy .. log_z, present, span skip, and log_z_free
    assert [float(t.flatten()[0]) for t in r[:4]] == [1.0, 1.125, 1.25, 1.375]
    assert [float(t.flatten()[0]) for t in r[4:10]] == [2.0, 2.125, 2.25, 2.375, 2.625, 2.75]
    assert float(r.log_z_free[0]) == (3.375 if has_win else 2.375)


def test_the_older_kinds_keep_their_routes_and_an_unknown_kind_is_refused(calls):
    from lyricalignment_amd.utils import alignment as ua
    em, lab, n_lab, nf, skip, win = _inputs(511)
    for conf, s, w, want in (("plain", None, None, ["viterbi_batch", "alignment_posteriors"]),
                             ("span", skip, None, ["viterbi_spans_batch", "alignment_posteriors_spans"]),
                             ("anchored", skip, win, ["viterbi_windows_batch", "alignment_posteriors_windows", "alignment_posteriors_spans"])):
        del calls[:]
        ua.run_lattice(em, lab, n_lab, nf, s, w, 1.5, conf, 2)
        assert [name for name, _, _ in calls] == want
    del calls[:]
    with pytest.raises(ValueError):
        ua.run_lattice(em, lab, n_lab, nf, None, None, 0.0, "song", 2)
    em, lab, n_lab, nf, skip, win = _inputs(512)
    with pytest.raises(NotImplementedError, match="511"):
        ua.run_lattice(em, lab, n_lab, nf, skip, win, 1.5, "anchored", 2)
    assert calls == []


# ------------------------------------------------------------------------------------------------ H4. surface refusals and align_song
@pytest.mark.parametrize("older", ["return_confidence", "return_span_confidence", "return_anchored_confidence"])
def test_sheet_confidence_does_not_go_with_an_older_confidence_keyword(older):
    from lyricalignment_amd.module.align_model import AlignModel
    model = AlignModel.__new__(AlignModel)                   # refused before the model is looked at
    with pytest.raises(ValueError, match="return_sheet_confidence"):
        AlignModel.align(model, [None], [[1, 2]], return_sheet_confidence=True, **{older: True})


class _StubModel:
    """Records what the sheet functions hand to AlignModel.align; one clip, every character 20 ms long, every score 0.5."""

    def __init__(self):
        self.calls = []

    def align(self, audios, labels, **kw):
        self.calls.append((labels.clone(), dict(kw)))
        n = labels.shape[1]
        res = [[[0.02 * j, 0.02 * j + 0.02] for j in range(n)]]
        if any(kw.get(k) for k in ("return_sheet_confidence", "return_anchored_confidence", "return_span_confidence")):
            return res, [dict(occupancy=[0.5] * n, onset_prob=[0.25] * n, offset_prob=[0.5] * n, sung_prob=[0.75] * n, span_skip_prob=[],
                              path_log_posterior=-1.0, window_log_prob=-0.125 if kw.get("onset_anchors") else 0.0)]
        return res


def test_align_song_builds_the_spans_and_anchors_of_the_existing_sheet_functions():
    from lyricalignment_amd import harness
    lines = ["ab", "cde", "f", "gh"]
    starts = [0.5, 1.25, 2.0, 61.5]
    optional = [False, True, False, True]
    lrc = "[ti:song]\n[00:00.50]ab\n[00:01.25]cde\n[00:02.00]f\n[01:01.50]gh\n"
    tokenize = lambda text: [ord(c) - 96 for c in text]
    lut = lambda ids: ids + 100
    audio = object()

    def keywords(f, *args, **kw):
        model = _StubModel()
        out = f(model, audio, *args, **kw)
        assert len(model.calls) == 1
        return model.calls[0], out

    (lab_lrc, kw_lrc), out_lrc = keywords(harness.align_record_lrc, list(zip(starts, lines)), lut, tokenize, tolerance_s=0.75, optional=optional,
                                          skip_penalty=0.5, with_confidence=True)
    (lab_lines, kw_lines), out_lines = keywords(harness.align_record_lines, lines, optional, lut, tokenize, skip_penalty=0.5)
    assert kw_lrc["optional_spans"] == kw_lines["optional_spans"] == [[(2, 5), (6, 8)]]
    assert kw_lrc["onset_anchors"] == [[(0, 0.5, 0.75), (2, 1.25, 0.75), (5, 2.0, 0.75), (6, 61.5, 0.75)]]
    for sheet in (lrc, list(zip(starts, lines)), [(s, l) for s, l in zip(starts, lines)]):
        (lab, kw), out = keywords(harness.align_song, sheet, lut, tokenize, tolerance_s=0.75, optional=optional, skip_penalty=0.5)
        assert torch.equal(lab, lab_lrc) and kw.pop("return_sheet_confidence") is True
        want = dict(kw_lrc)
        want.pop("return_anchored_confidence")
        assert kw == want
        assert out == out_lrc and out[1] == {"sung": [0.75] * 4, "line_onset_prob": [0.25] * 4, "window_log_prob": -0.125}
    (lab, kw), out = keywords(harness.align_song, lines, lut, tokenize, optional=optional, skip_penalty=0.5)     # plain lines: no anchors
    assert torch.equal(lab, lab_lines) and kw.pop("return_sheet_confidence") is True and "onset_anchors" not in kw
    assert kw == kw_lines
    assert out[0] == out_lines and out[1]["window_log_prob"] == 0.0 and out[1]["sung"] == [0.75] * 4
    (_, kw), _ = keywords(harness.align_song, lines, lut, tokenize)                                              # optional defaults to none
    assert kw["optional_spans"] == [[]] and kw["skip_penalty"] == 0.0 and kw["use_ctc"] is True
    for bad in ([], "", "[ti:no timed line]"):
        with pytest.raises(ValueError, match="align_song"):
            harness.align_song(_StubModel(), audio, bad, lut, tokenize)
    with pytest.raises(ValueError, match="align_song"):
        harness.align_song(_StubModel(), audio, lines, lut, lambda text: [1])
