"""Host side of the pronunciation alternatives (la_emissions_merge_readings / la_reading_scores; ops.merge_readings / ops.reading_scores;
utils.alignment._readings_of; the `alternatives` / `return_readings` keywords; PinyinClassLUT.readings_of): the helper's outputs and every
refusal, the float64 fold of the yardstick, the declarations, every argument error of the two entries under their own names, and the
Python refusals that need no device.  The numbers are tested on the GPU (tests/test_gpu_readings.py)."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import readings_reference as rdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("la_emissions_merge_readings", "la_reading_scores")


def _ua():
    from lyricalignment_amd.utils import alignment as ua
    return ua


def test_the_helper_builds_expanded_labels_csr_rows_ids_and_column_counts():
    ua = _ua()
    lists = [[3, 5, 5, 9], [7], []]
    rd = ua._readings_of([[(1, [8, 2]), (3, [4])], [(0, [1, 2, 3, 4, 5, 6, 8])], []], lists)
    assert rd.n_columns == [7, 8, 0]
    assert rd.labels_x.dtype == torch.int32 and rd.labels_x.shape == (3, 8)
    assert rd.labels_x[0, :7].tolist() == [3, 5, 8, 2, 5, 9, 4] and rd.labels_x[1].tolist() == [7, 1, 2, 3, 4, 5, 6, 8]
    assert rd.alt_start.dtype == torch.int32 and rd.alt_start.shape == (3, 5)
    assert rd.alt_start.tolist() == [[0, 1, 4, 5, 7], [0, 8, 8, 8, 8], [0, 0, 0, 0, 0]]          # past L_b: the last value
    assert rd.lattice_ids.tolist() == [[3, ua.READING_SET_ID, 5, ua.READING_SET_ID + 1], [ua.READING_SET_ID, 0, 0, 0], [0, 0, 0, 0]]
    assert rd.sets[0] == [[3], [5, 8, 2], [5], [9, 4]] and rd.sets[2] == []
    for b, row in enumerate(rd.sets):
        assert rd.lattice_ids[b, : len(row)].tolist() == rdr.lattice_ids(row)
    assert ua.READING_SET_ID == rdr.READING_SET_ID == 1 << 24


def test_none_and_all_empty_return_none_and_ids_equal_the_labels_without_extras():
    ua = _ua()
    lists = [[3, 5, 5], [2, 2]]
    assert ua._readings_of(None, lists) is None
    assert ua._readings_of([[], []], lists) is None and ua._readings_of([None, ()], lists) is None
    rd = ua._readings_of([[], []], lists, keep_empty=True)
    assert rd.lattice_ids.tolist() == [[3, 5, 5], [2, 2, 0]] and rd.labels_x.tolist() == [[3, 5, 5], [2, 2, 0]]
    assert rd.alt_start.tolist() == [[0, 1, 2, 3], [0, 1, 2, 2]] and rd.n_columns == [3, 2]
    assert ua._readings_of(None, lists, keep_empty=True) is None


def test_equal_sets_get_equal_ids_and_overlapping_different_sets_different_ones():
    ua = _ua()
    lists = [[3, 8, 3, 3, 8, 6]]
    rd = ua._readings_of([[(0, [8]), (1, [3]), (2, [8, 9]), (3, [9]), (4, [3]), (5, [3])]], lists)
    ids = rd.lattice_ids[0].tolist()
    assert ids[0] == ids[1] == ids[4]                       # {3, 8} in either order, the sheet's class different: one set, one id
    assert ids[2] != ids[0] and ids[3] != ids[0] and ids[2] != ids[3]          # {3, 8, 9} and {3, 9} overlap {3, 8} and differ
    assert ids[5] not in ids[:5] and all(i >= ua.READING_SET_ID for i in ids)
    assert ids == rdr.lattice_ids(rd.sets[0]) == [ua.READING_SET_ID + k for k in (0, 0, 1, 2, 0, 3)]


def test_every_refusal_of_the_helper():
    ua = _ua()
    lists = [[3, 5, 7]]
    for bad in ([[], []],                                       # a wrong list count
                [[(3, [4])]], [[(-1, [4])]], [[(1.5, [4])]],     # n outside 0 .. L-1
                [[(1, [4]), (1, [6])]],                          # two entries for one n
                [[(1, [])]],                                     # an empty extras list
                [[(1, [4, 4])]], [[(1, [5])]],                   # a class repeated within a set, the sheet's own included
                [[(1, [10, 11, 12, 13, 14, 15, 16, 17])]]):      # nine readings
        with pytest.raises(ValueError):
            ua._readings_of(bad, lists)
    assert ua._readings_of([[(1, [10, 11, 12, 13, 14, 15, 16])]], lists).n_columns == [10]         # eight are taken
    wide = [list(range(2, 2050))]                               # 2048 labels: 2047 with two readings = 4095 columns, one more = 4096
    assert ua._readings_of([[(n, [1]) for n in range(2047)]], wide).n_columns == [4095]
    with pytest.raises(NotImplementedError):
        ua._readings_of([[(n, [1]) for n in range(2048)]], wide)
    assert ua.MAX_READINGS == 8 and ua.MAX_READING_COLUMNS == 4095


def test_the_float64_fold_equals_the_log_of_the_summed_probabilities():
    rs = np.random.RandomState(3)
    for A in (2, 3, 8):
        for _ in range(20):
            x = (-rs.rand(A) * 12.0).astype(np.float32)
            direct = math.log(sum(math.exp(float(v)) for v in x))
            assert abs(float(rdr.fold64(x)) - direct) <= 1e-14 * max(1.0, abs(direct))
    assert rdr.fold64([np.float32(-2.5)]) == np.float64(np.float32(-2.5))
    assert rdr.fold64([-np.inf, -np.inf]) == -np.inf and rdr.fold64([-np.inf, np.float32(-3.0)]) == -3.0
    assert rdr.fold64([np.float32(-1000.0)] * 2) == -1000.0 + math.log(2.0)
    assert rdr.fold64([np.float32(-5.0), np.float32(-95.0)]) == -5.0 + math.log(1.0 + math.exp(-90.0))
    # the row form is the scalar form, frame by frame, and its rounded form is that rounded once
    em_x = (-rs.rand(6, 7) * 9.0).astype(np.float32)
    em_x[2, 3:5] = -np.inf
    alt = [0, 1, 4, 6]
    rows = rdr.fold_rows64(em_x, alt)
    for t in range(6):
        assert rows[t, 0] == em_x[t, 0] and rows[t, 1] == em_x[t, 1]
        for n in (1, 2):
            want = rdr.fold64(em_x[t, 1 + alt[n]: 1 + alt[n + 1]])
            assert rows[t, 1 + n] == want or abs(rows[t, 1 + n] - want) <= 4 * np.spacing(abs(want))
    assert rdr.fold_rows(em_x, alt).dtype == np.float32 and (rdr.fold_rows(em_x, alt) == rows.astype(np.float32)).all()
    # the sequential sums and the reading rule: the smallest index wins a tie, a skipped position gives -1 and zeros
    sc = rdr.segment_scores(em_x, alt, [0, 2, -1], [2, 6, -1])
    assert sc[0] == float(em_x[0, 1]) + float(em_x[1, 1]) and sc[4] == 0.0 and sc[5] == 0.0 and sc[2] == -np.inf
    assert rdr.pick_readings(sc, alt, [0, 2, -1]) == [0, 0, -1]
    assert rdr.pick_readings(np.array([0.0, -3.0, -1.0, -1.0, -2.0, -1.5]), alt, [0, 1, 2]) == [0, 1, 1]


def test_the_entry_points_are_declared_and_exported():
    from lyricalignment_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lyricalign.h")).read(), flags=re.S)
    for name in ENTRIES:
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert decl, f"{name} not declared in lyricalign.h"
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == decl.group(1).count(",") + 1
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} not exported"
    assert callable(ops.merge_readings) and callable(ops.reading_scores)


def test_every_argument_error_is_answered_on_the_host_under_the_entrys_name():
    from lyricalignment_amd import _lib
    L = _lib.lib()
    P = 16                                      # a non-null stand-in pointer: every call below is refused before any device call
    T, Lmax, X = 100, 26, 40

    def merge(em_x=P, xbs=None, xrs=X + 1, alt=P, alt_stride=Lmax + 1, n_labels=P, n_frames=P, batch=2, T=T, Lmax=Lmax, X=X, em=P, ebs=None,
              ers=Lmax + 1):
        return L.la_emissions_merge_readings(em_x, T * xrs if xbs is None else xbs, xrs, alt, alt_stride, n_labels, n_frames, batch, T, Lmax, X,
                                             em, T * ers if ebs is None else ebs, ers, 0)

    def scores(em_x=P, xbs=None, xrs=X + 1, alt=P, alt_stride=Lmax + 1, n_labels=P, onset=P, offset=P, out_stride=Lmax, batch=2, T=T, Lmax=Lmax,
               X=X, col_score=P, col_stride=X, reading=P, reading_stride=Lmax):
        return L.la_reading_scores(em_x, T * xrs if xbs is None else xbs, xrs, alt, alt_stride, n_labels, onset, offset, out_stride, batch, T,
                                   Lmax, X, col_score, col_stride, reading, reading_stride, 0)

    def refused(call, who, what, rc=_lib.LA_EINVAL, **kw):
        assert call(**kw) == rc, kw
        assert what in _lib.last_error() and who in _lib.last_error(), (kw, _lib.last_error())

    for call, who, pointers, own in ((merge, "emissions_merge_readings", ("em_x", "alt", "n_labels", "n_frames", "em"), dict(ers=Lmax)),
                                     (scores, "reading_scores", ("em_x", "alt", "n_labels", "onset", "offset", "col_score", "reading"),
                                      dict(out_stride=Lmax - 1))):
        for null in pointers:
            refused(call, who, "null", **{null: 0})
        for size in ("batch", "T", "Lmax"):
            refused(call, who, "sizes", **{size: 0})
            refused(call, who, "sizes", **{size: -1})
        refused(call, who, "max_columns", X=Lmax - 1, xrs=X + 1)
        refused(call, who, "strides", xrs=X)
        refused(call, who, "strides", alt_stride=Lmax)
        refused(call, who, "strides", xbs=(T - 1) * (X + 1) + X)
        refused(call, who, "strides", **own)
        # the limits: reported before the strides
        refused(call, who, "4095", rc=_lib.LA_EUNSUPPORTED, X=4096, xrs=1)
        refused(call, who, "4095", rc=_lib.LA_EUNSUPPORTED, Lmax=4096, X=4096, alt_stride=1)
    refused(merge, "emissions_merge_readings", "strides", ebs=(T - 1) * (Lmax + 1) + Lmax)
    refused(scores, "reading_scores", "strides", reading_stride=Lmax - 1)
    refused(scores, "reading_scores", "strides", col_stride=X - 1)


def test_python_refusals_that_need_no_device():
    from lyricalignment_amd.finetune import FineTuner
    from lyricalignment_amd.harness import PinyinClassLUT, align_record_lines, align_record_lrc, align_song
    from lyricalignment_amd.module.align_model import AlignModel
    ua = _ua()
    logits = torch.zeros((1, 20, 12))
    labels = torch.tensor([[3, 5, 7]])
    family = [getattr(ua, "perform_viterbi" + ctc + kind) for ctc in ("", "_ctc")
              for kind in ("", "_scored", "_anchored_scored", "_sheet_scored", "_repeat_scored", "_song_scored")]
    for f in family:
        sig = inspect.signature(f).parameters
        assert sig["alternatives"].default is None and sig["return_readings"].default is False, f.__name__
        with pytest.raises(ValueError, match="return_readings"):                  # return_readings without alternatives
            f(logits, labels, return_readings=True)

    class Unbuilt(AlignModel):                                          # align's keyword checks come before the engine exists
        def __init__(self):
            pass

        def engine(self):
            raise AssertionError("the refusal comes before anything is on a device")

    audio = [np.zeros(16000, np.float32)]
    with pytest.raises(ValueError, match="return_readings"):
        AlignModel.align(Unbuilt(), audio, labels, return_readings=True)
    for bad in ([[(3, [4])]], [[(1, [5])]], [[(1, [])]], [[], []], [[(0, list(range(10, 18)))]]):
        with pytest.raises(ValueError):
            AlignModel.align(Unbuilt(), audio, labels, alternatives=bad)
    with pytest.raises(NotImplementedError):
        AlignModel.align(Unbuilt(), audio, torch.arange(2, 2050)[None], alternatives=[[(n, [1]) for n in range(2048)]])
    with pytest.raises(AssertionError):                                 # good alternatives are accepted (and go on to the engine)
        AlignModel.align(Unbuilt(), audio, labels, alternatives=[[(1, [4])]], return_readings=True)
    sig = inspect.signature(AlignModel.align).parameters
    assert sig["alternatives"].default is None and sig["return_readings"].default is False
    assert "alternatives" in AlignModel.align.__doc__ and "return_readings" in AlignModel.align.__doc__

    # training on merged classes is not part of this
    with pytest.raises(ValueError, match="alternatives"):
        ua.anchored_alignment_loss(logits, labels, alternatives=[[(1, [4])]])
    with pytest.raises(ValueError, match="alternatives"):
        FineTuner.micro_step_anchored(object(), audio, labels, alternatives=[[(1, [4])]])

    # the heteronym dict of the harness: syllables resolved through the lookup table, the table's own class and repeats dropped
    lut = PinyinClassLUT(["de", "le", "a", "zhe"], {"de": 3, "le": 5, "a": 7, "zhe": 9, "di": 4, "liao": 6, "zhao": 8})
    tokens = torch.tensor([[0, 2, 1, -100], [3, 3, -100, -100]])
    assert lut(tokens).tolist() == [[3, 7, 5, -100], [9, 9, -100, -100]]
    assert lut.readings_of(tokens, {0: ["di", "de"], 1: ["liao", "liao"], 3: ["zhao", "zhe"]}) == [[(0, [4]), (2, [6])], [(0, [8]), (1, [8])]]
    assert lut.readings_of(tokens, {}) == [[], []]
    with pytest.raises(ValueError, match="xx"):
        lut.readings_of(tokens, {0: ["xx"]})
    for f in (align_record_lines, align_record_lrc, align_song):
        assert inspect.signature(f).parameters["heteronyms"].default is None
