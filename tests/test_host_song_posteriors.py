"""Host side of the whole-song repeat confidence (la_alignment_posteriors_song; ops.alignment_posteriors_song; run_lattice's "song";
AlignModel.align(return_song_confidence=True); harness.align_song(repeatable=...)): declarations, the documented workspace size, every
argument error of the entry under its own name, and the Python refusals that need no device.  The numbers are tested on the GPU
(tests/test_gpu_song_posteriors.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import song_posterior_cases as spc
import wide_posterior_cases as wpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = "alignment_posteriors_song"


def test_the_entry_points_are_declared_and_exported():
    from lyricalignment_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lyricalign.h")).read(), flags=re.S)
    for name in ("la_alignment_posteriors_song_workspace_bytes", "la_alignment_posteriors_song"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in lyricalign.h"
        assert name in _lib.SYMBOLS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} not exported"
    # the arguments are the repeats entry's, unchanged and in the same order
    decl = {n: re.search(r"\bint\s+la_" + n + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1) for n in (WHO, "alignment_posteriors_repeats")}
    assert re.sub(r"\s+", " ", decl[WHO]) == re.sub(r"\s+", " ", decl["alignment_posteriors_repeats"])
    assert _lib.SYMBOLS["la_" + WHO] == _lib.SYMBOLS["la_alignment_posteriors_repeats"]


def test_the_workspace_query():
    from lyricalignment_amd import _lib
    L = _lib.lib()
    f = L.la_alignment_posteriors_song_workspace_bytes
    need, old = ctypes.c_size_t(1), ctypes.c_size_t(2)
    for shape in ((1, 600, 512), (1, 12000, 2500), (2, 50, 4095)):
        assert f(*shape, ctypes.byref(need)) == _lib.LA_OK and need.value == spc.workspace_bytes(*shape), shape
    B, T, Lmax = 1, 12000, 2500                    # the documented formula, written out once: R = 8, NS = 8192
    assert spc.workspace_bytes(B, T, Lmax) == B * T * 8192 * 8 + B * 4096 * 6 * 8 + B * 3 * 8192 * 4
    for shape in ((32, 1500, 26), (1, 600, 511)):
        assert f(*shape, ctypes.byref(need)) == _lib.LA_OK
        assert L.la_alignment_posteriors_repeats_workspace_bytes(*shape, ctypes.byref(old)) == _lib.LA_OK and need.value == old.value
        assert need.value == spc.workspace_bytes(*shape)
    assert f(1, 600, 4096, ctypes.byref(need)) == _lib.LA_EUNSUPPORTED
    assert "4095" in _lib.last_error() and WHO in _lib.last_error()
    assert f(1, 600, 26, None) == _lib.LA_EINVAL and WHO in _lib.last_error()
    assert f(1, 0, 26, ctypes.byref(need)) == _lib.LA_EINVAL and f(1, 600, 0, ctypes.byref(need)) == _lib.LA_EINVAL


@pytest.mark.parametrize("Lmax", [26, 600])
def test_every_argument_error_is_answered_on_the_host_under_the_entrys_name(Lmax):
    from lyricalignment_amd import _lib
    L = _lib.lib()
    P = 16                                      # a non-null, aligned stand-in pointer: every call below is refused before any device call
    big = 1 << 40
    T = 100

    def call(em=P, labels=P, n_labels=P, n_frames=P, batch=2, T=T, Lmax=Lmax, onset=P, offset=P, out_stride=Lmax, bw=2, skip_from=P,
             skip_stride=Lmax + 1, penalty=0.0, win_lo=P, win_hi=P, win_stride=2 * Lmax + 1, repeat_from=P, repeat_stride=Lmax,
             repeat_penalty=0.0, path=P, path_stride=T, occupancy=P, onset_prob=P, offset_prob=P, visits=P, span_skip_prob=P, repeat_count=P,
             path_prob=P, log_z=P, status=P, gamma=0, gamma_bs=0, gamma_rs=0, ws=P, ws_bytes=big, em_rs=Lmax + 1, labels_stride=Lmax):
        return L.la_alignment_posteriors_song(em, T * em_rs, em_rs, labels, labels_stride, n_labels, n_frames, batch, T, Lmax, onset, offset,
                                              out_stride, bw, skip_from, skip_stride, penalty, win_lo, win_hi, win_stride, repeat_from,
                                              repeat_stride, repeat_penalty, path, path_stride, occupancy, onset_prob, offset_prob, visits,
                                              span_skip_prob, repeat_count, path_prob, log_z, status, gamma, gamma_bs, gamma_rs, ws, ws_bytes, 0)

    def refused(what, **kw):
        assert call(**kw) == _lib.LA_EINVAL, kw
        assert what in _lib.last_error() and WHO in _lib.last_error(), (kw, _lib.last_error())

    for null in ("em", "labels", "n_labels", "n_frames", "onset", "offset", "occupancy", "onset_prob", "offset_prob", "visits",
                 "span_skip_prob", "repeat_count", "log_z", "status"):
        refused("null", **{null: 0})
    refused("go together", win_lo=0)
    refused("go together", win_hi=0)
    refused("strides", win_stride=2 * Lmax)
    refused("strides", skip_stride=Lmax)
    refused("strides", out_stride=Lmax - 1)
    refused("strides", em_rs=Lmax)
    refused("strides", labels_stride=Lmax - 1)
    refused("skip_penalty", penalty=-0.5)
    refused("skip_penalty", penalty=float("nan"))
    refused("boundary_window", bw=-1)
    refused("repeat_penalty", repeat_penalty=-0.5)
    refused("repeat_penalty", repeat_penalty=float("nan"))
    refused("repeat_stride", repeat_stride=Lmax - 1)
    refused("path_stride", path_stride=T - 1)
    refused("path_prob", path=0)                                   # path_prob without path
    refused("path_stride", path_prob=0, path_stride=T - 1)        # a path alone is checked too
    refused("gamma", gamma=P, gamma_bs=T * (2 * Lmax + 1), gamma_rs=2 * Lmax)
    refused("gamma", gamma=P, gamma_bs=T * (2 * Lmax + 1) - 1, gamma_rs=2 * Lmax + 1)
    refused("sizes", T=0)
    refused("sizes", Lmax=0)
    refused("sizes", batch=-1)
    refused("workspace too small", ws_bytes=spc.workspace_bytes(2, T, Lmax) - 1)
    refused("workspace", ws=0)
    refused("aligned", ws=24)                                      # 16-byte alignment, at every label count
    assert call(ws_bytes=spc.workspace_bytes(2, T, Lmax), batch=0) == _lib.LA_OK          # nothing to do, nothing enqueued
    # the label limit: reported before the strides
    assert call(Lmax=4096, out_stride=1) == _lib.LA_EUNSUPPORTED and "4095" in _lib.last_error() and WHO in _lib.last_error()
    # the optional inputs may each be absent: refused only further on (here: by the missing workspace)
    refused("workspace", skip_from=0, win_lo=0, win_hi=0, repeat_from=0, path=0, path_prob=0, repeat_stride=0, path_stride=0, win_stride=0, ws=0)


def test_python_refusals_that_need_no_device():
    import torch
    from lyricalignment_amd import ops
    from lyricalignment_amd.harness import PinyinClassLUT, align_song
    from lyricalignment_amd.module.align_model import AlignModel
    from lyricalignment_amd.utils import alignment as ua
    rows = torch.zeros((1, 600), dtype=torch.int32)
    wide = torch.zeros((1, 600), dtype=torch.int32)
    for kind in ("plain", "span", "anchored", "sheet"):                 # the older kinds keep refusing the repeat lattice, wide or not
        with pytest.raises(ValueError):
            ua.run_lattice(None, wide, None, None, confidence=kind, repeat_from=rows)
    with pytest.raises(ValueError):
        ua.run_lattice(None, wide, None, None, confidence="songs")
    with pytest.raises(NotImplementedError):                            # "repeat" keeps its limit
        ua.run_lattice(None, wide, None, None, confidence="repeat", repeat_from=rows)
    assert "song" in inspect.getsource(ua.run_lattice) and callable(ops.alignment_posteriors_song)
    assert inspect.signature(ops.alignment_posteriors_song) == inspect.signature(ops.alignment_posteriors_repeats)
    for name in ("perform_viterbi_song_scored", "perform_viterbi_ctc_song_scored"):
        assert inspect.signature(getattr(ua, name)) == inspect.signature(getattr(ua, name.replace("song", "repeat")))

    class Unbuilt(AlignModel):                                          # align's keyword checks come before the engine exists
        def __init__(self):
            pass

        def engine(self):
            raise AssertionError("the refusal comes before anything is on a device")

    labels = torch.ones((1, 600), dtype=torch.int64)
    for other in ("return_confidence", "return_span_confidence", "return_anchored_confidence", "return_sheet_confidence",
                  "return_repeat_confidence"):
        with pytest.raises(ValueError):
            AlignModel.align(Unbuilt(), [np.zeros(16000, np.float32)], labels, return_song_confidence=True, **{other: True})
    with pytest.raises(AssertionError):                                 # alone it is accepted at 600 labels (and goes on to the engine)
        AlignModel.align(Unbuilt(), [np.zeros(16000, np.float32)], labels, return_song_confidence=True)

    lut = PinyinClassLUT([str(i) for i in range(8)], {str(i): i for i in range(8)})
    lines = ["ab", "cde", "f"]
    for flags in ([True], [False, True], [False, True, False, False]):
        with pytest.raises(ValueError, match="repeatable"):
            align_song(Unbuilt(), np.zeros(16000, np.float32), lines, lut, lambda t: [1] * len(t), repeatable=flags)
    sig = inspect.signature(align_song).parameters
    assert sig["repeatable"].default is None and sig["repeat_penalty"].default == 0.0
    assert "return_song_confidence" in inspect.signature(AlignModel.align).parameters


def test_the_helper_sheets_hold_what_they_are_meant_to():
    """The arc lists of song_posterior_cases.mixed_sheet, on the host: one thread folds more than four words, skip words followed by
    repeat words for one state, and its wave mates fold fewer."""
    for L in (512, 1024, 2048):
        skip, rf, sung = spc.mixed_sheet(L)
        lab = wpc.labels_of(L, L)
        R = wpc.strip_states_per_thread(L)
        assert spc.assert_mixed_arc_lists(skip, rf, lab, R) >= 8
        assert sorted(set(sung)) == list(range(L)) and sum(y <= x for x, y in zip(sung, sung[1:])) == 4
        assert {101, 107, 115, 118} <= set(spc.breaths_of(lab, sung))
        reps = spc.repeat_arc_words(rf, lab, R)
        assert reps[202] == [191, 195] and reps[210] == [207] and reps[212] == [209]      # two spans share the end 101; adjacent ends
