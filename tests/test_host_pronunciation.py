"""Host side of the pronunciation scores (la_segment_class_scores; ops.segment_class_scores; utils.alignment._pronunciation_of /
_widened_labels / _own_columns; the return_pronunciation / pronunciation_classes / pronunciation_top_k keywords; the harness's
with_pronunciation and suspect_characters): the keyword checks and every refusal, the widened label rows and own columns, the
declaration, every argument error of the entry under its own name, the restatement against brute-force enumeration, and that a call
without the keyword builds exactly the rows it builds today.  The numbers are tested on the GPU (tests/test_gpu_pronunciation.py)."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

import pronunciation_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "la_segment_class_scores"


def _ua():
    from lyricalignment_amd.utils import alignment as ua
    return ua


def test_the_keywords_give_a_sorted_unique_class_list_with_the_sheets_own_classes():
    ua = _ua()
    lists = [[30, 5, 5, 46], [7], []]
    assert ua._pronunciation_of("who", False, None, 5, lists) is None and ua._pronunciation_of("who", False, 40, 99, lists) is None
    p = ua._pronunciation_of("who", True, 8, 5, lists)
    assert p.classes == [1, 2, 3, 4, 5, 6, 7, 8, 30, 46] == pr.candidate_classes(8, lists) and p.top_k == 5
    assert p.own_col.dtype == torch.int32 and p.own_col.tolist() == [[8, 4, 4, 9], [6, -1, -1, -1], [-1, -1, -1, -1]]
    assert p.col_of.dtype == torch.int32 and p.col_of.shape == (47,) and p.col_of[30] == 8 and p.col_of[0] == -1 and p.col_of[29] == -1
    q = ua._pronunciation_of("who", True, [46, 9, 9, 2], 16, lists)
    assert q.classes == [2, 5, 7, 9, 30, 46] == pr.candidate_classes([46, 9, 9, 2], lists) and q.top_k == 16
    q = ua._pronunciation_of("who", True, np.array([3, 1]), 1, [[2]])
    assert q.classes == [1, 2, 3] and q.own_col.tolist() == [[1]]
    # with alternatives every reading's class is a candidate, and the width that counts is the widest expanded row
    rd = ua._readings_of([[(1, [8, 2])], [], []], lists)
    r = ua._pronunciation_of("who", True, [1], 5, lists, rd)
    assert r.classes == [1, 2, 5, 7, 8, 30, 46] and r.own_col.tolist()[0] == [5, 2, 2, 6]


def test_every_refusal_of_the_keywords():
    ua = _ua()
    lists = [[3, 5, 7]]
    with pytest.raises(ValueError, match="pronunciation_classes"):                  # the missing class list
        ua._pronunciation_of("who", True, None, 5, lists)
    for top_k in (0, -1, 17, 2.5, True):
        with pytest.raises(ValueError, match="pronunciation_top_k"):
            ua._pronunciation_of("who", True, 10, top_k, lists)
    for bad in (0, -3, [0, 4], [-1]):
        with pytest.raises(ValueError, match="class"):
            ua._pronunciation_of("who", True, bad, 5, lists)
    assert ua.MAX_PRONUNCIATION_COLUMNS == 4095
    assert len(ua._pronunciation_of("who", True, 4092, 5, lists).classes) == 4092                  # 3 + 4092 = 4095 columns are taken
    with pytest.raises(NotImplementedError, match="4095"):
        ua._pronunciation_of("who", True, 4093, 5, lists)
    wide = [list(range(1, 601))]
    assert len(ua._pronunciation_of("who", True, 3495, 5, wide).classes) == 3495
    with pytest.raises(NotImplementedError):
        ua._pronunciation_of("who", True, 3496, 5, wide)
    rd = ua._readings_of([[(0, [9, 10])]], lists)                                     # five expanded columns
    assert len(ua._pronunciation_of("who", True, 4090, 5, lists, rd).classes) == 4090
    with pytest.raises(NotImplementedError):
        ua._pronunciation_of("who", True, 4091, 5, lists, rd)


def test_the_widened_rows_and_the_own_columns():
    ua = _ua()
    lab = torch.tensor([[30, 5, 5, 46], [7, 0, 0, 0], [0, 0, 0, 0]], dtype=torch.int32)
    n = torch.tensor([4, 1, 0], dtype=torch.int32)
    classes = torch.tensor([2, 5, 7, 30, 46], dtype=torch.int32)
    lab_w, n_w = ua._widened_labels(lab, n, classes)
    assert lab_w.dtype == torch.int32 and lab_w.is_contiguous() and n_w.dtype == torch.int32
    assert lab_w.tolist() == [[30, 5, 5, 46, 2, 5, 7, 30, 46], [7, 2, 2, 2, 2, 5, 7, 30, 46], [2, 2, 2, 2, 2, 5, 7, 30, 46]]
    assert n_w.tolist() == [9, 9, 9]                                  # every clip asks for all columns: the candidates sit at fixed ones
    # the own columns: the sheet's class without alternatives; with them the reading that was picked, -1 for a skipped position
    lists = [[30, 5, 5, 46], [7], []]
    p = ua._pronunciation_of("who", True, [2], 5, lists)
    assert ua._own_columns(p, None, None, torch.device("cpu")).tolist() == p.own_col.tolist() == [[3, 1, 1, 4], [2, -1, -1, -1], [-1] * 4]
    rd = ua._readings_of([[(1, [8, 2]), (3, [4])], [], []], lists)
    p = ua._pronunciation_of("who", True, [2], 5, lists, rd)
    assert p.classes == [2, 4, 5, 7, 8, 30, 46]
    route = ua.ReadingRoute(rd, None, rd.alt_start, None, rd.lattice_ids)
    reading = torch.tensor([[0, 2, -1, 1], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=torch.int32)
    assert ua._own_columns(p, route, reading, torch.device("cpu")).tolist() == [[5, 0, -1, 1], [3, -1, -1, -1], [-1] * 4]


def test_the_public_dicts_from_the_entrys_outputs():
    ua = _ua()
    lists = [[30, 5, 9]]
    p = ua._pronunciation_of("who", True, [2], 2, lists)               # classes [2, 5, 9, 30]
    top_col = torch.tensor([[[3, 0], [2, 1], [-1, -1]]], dtype=torch.int32)
    top_score = torch.tensor([[[-4.0, -8.0], [-3.0, -9.0], [0.0, 0.0]]], dtype=torch.float64)
    own_score = torch.tensor([[-4.0, -9.0, 0.0]], dtype=torch.float64)
    own_rank = torch.tensor([[0, 1, -1]], dtype=torch.int32)
    n_seg = torch.tensor([[4, 3, 0]], dtype=torch.int32)
    got = ua._pronunciation_from_scores((top_col, top_score, own_score, own_rank, n_seg), p.own_col, p, lists)
    assert got == [[{"class": 30, "frames": 4, "log_prob": -1.0, "rank": 0, "gop": 0.0, "top": [(30, -1.0), (2, -2.0)]},
                    {"class": 5, "frames": 3, "log_prob": -3.0, "rank": 1, "gop": -2.0, "top": [(9, -1.0), (5, -3.0)]}, None]]
    ref = {"top_col": top_col.numpy(), "top_score": top_score.numpy(), "own_score": own_score.numpy(), "own_rank": own_rank.numpy(),
           "n_seg_frames": n_seg.numpy()}
    assert got[0] == pr.pronunciation_dicts(ref, 0, lists[0], p.classes)


def test_the_restatement_equals_brute_force_enumeration_on_tiny_inputs():
    rs = np.random.RandomState(4)
    for C, T in ((1, 3), (3, 4), (4, 5)):
        em = rs.randint(-3, 1, size=(T, C)).astype(np.float32)          # small integers: exact sums, many ties
        em[rs.rand(T, C) < 0.15] = -np.inf
        for t0, t1 in ((0, T), (1, 2), (T - 1, T + 4), (2, 2)):
            sums, frames = pr.segment_sums(em, t0, t1)
            u = min(t1, T)
            assert frames == max(0, u - t0)
            for j in range(C):                                          # a plain Python float loop per column
                s = 0.0
                for t in range(t0, u):
                    s += float(em[t, j])
                assert sums[j] == s
            for own in range(C):
                for top_k in (1, C, C + 2):
                    tc, ts, own_score, rank = pr.select(sums, own, top_k)
                    # brute force: the one permutation of the columns in which every neighbour pair is in order
                    orders = [o for o in itertools.permutations(range(C))
                              if all(sums[a] > sums[b] or (sums[a] == sums[b] and a < b) for a, b in zip(o, o[1:]))]
                    assert len(orders) == 1
                    assert tc == list(orders[0][:top_k]) + [-1] * max(0, top_k - C)
                    assert ts[:C] == [float(sums[j]) for j in orders[0][:top_k]] and all(v == -np.inf for v in ts[C:])
                    assert rank == orders[0].index(own) == pr.rank_by_count(sums, own) and own_score == sums[own]
            assert pr.select(sums, -1, 2)[2:] == (0.0, -1)
    # the batch form: ragged label counts, a skipped position, what lies beyond a clip's labels keeps the caller's fill
    em = rs.randint(-3, 1, size=(2, 6, 3)).astype(np.float32)
    ref = pr.segment_class_scores(em, [2, 1], [[0, -1], [2, 9]], [[3, -1], [6, 9]], [[1, 2], [0, 0]], 2, fill={"top_col": -7, "own_rank": -7})
    assert ref["own_rank"][0, 1] == -1 and ref["top_col"][0, 1].tolist() == [-1, -1] and ref["n_seg_frames"].tolist() == [[3, 0], [4, 0]]
    assert ref["top_col"][1, 1].tolist() == [-7, -7] and ref["own_rank"][1, 1] == -7 and (ref["seg_score"][0, 1] == 0.0).all()
    assert ref["seg_score"][1, 0].tolist() == [float(sum(float(v) for v in em[1, 2:6, j])) for j in range(3)]


def test_the_entry_point_is_declared_and_exported():
    from lyricalignment_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lyricalign.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + ENTRY + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert decl, f"{ENTRY} not declared in lyricalign.h"
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert _lib.SYMBOLS[ENTRY] == (I32, [P, I64, I64, P, P, P, I32, P, I32, I32, I32, I32, I32, I32, P, I64, I64, P, P, I32, P, P, P, P])
    assert len(_lib.SYMBOLS[ENTRY][1]) == decl.group(1).count(",") + 1 == 24
    kinds = [I64 if "int64_t" in a else I32 if "int32_t" in a and "*" not in a else P for a in decl.group(1).split(",")]
    assert kinds == _lib.SYMBOLS[ENTRY][1]                              # the ctypes signature is the declaration's, argument by argument
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), ENTRY), f"{ENTRY} not exported"
    assert callable(ops.segment_class_scores) and ops.MAX_PRONUNCIATION_TOP_K == 16
    sig = inspect.signature(ops.segment_class_scores).parameters
    assert list(sig)[:7] == ["em_c", "n_labels", "onset", "offset", "own_col", "top_k", "want_scores"]
    assert sig["top_k"].default == 5 and sig["want_scores"].default is False


def test_every_argument_error_is_answered_on_the_host_under_the_entrys_name():
    from lyricalignment_amd import _lib
    L = _lib.lib()
    P = 16                                      # a non-null stand-in pointer: every call below is refused before any device call
    T, Lmax, C, K = 100, 26, 402, 5
    good = dict(em_c=P, ebs=T * C, ers=C, n_labels=P, onset=P, offset=P, out_stride=Lmax, own_col=P, own_stride=Lmax, batch=2, T=T, Lmax=Lmax,
                C=C, top_k=K, seg=P, sbs=Lmax * C, srs=C, top_col=P, top_score=P, top_stride=K, own_score=P, own_rank=P, n_seg=P)

    def refused(what, rc=_lib.LA_EINVAL, **kw):
        a = {**good, **kw}
        assert L.la_segment_class_scores(*(a[k] for k in good), 0) == rc, kw
        assert what in _lib.last_error() and "segment_class_scores" in _lib.last_error(), (kw, _lib.last_error())

    for null in ("em_c", "n_labels", "onset", "offset", "own_col", "top_col", "top_score", "own_score", "own_rank", "n_seg"):
        refused("null", **{null: 0})
    for size in ("batch", "T", "Lmax", "C", "top_k"):
        refused("sizes", **{size: 0})
        refused("sizes", **{size: -1})
    for kw in (dict(ers=C - 1), dict(ebs=(T - 1) * C + C - 1), dict(out_stride=Lmax - 1), dict(own_stride=Lmax - 1), dict(top_stride=K - 1),
               dict(srs=C - 1), dict(sbs=(Lmax - 1) * C + C - 1)):
        refused("strides", **kw)
    # the limits: reported before the strides
    refused("4095", rc=_lib.LA_EUNSUPPORTED, C=4096, ers=1)
    refused("4095", rc=_lib.LA_EUNSUPPORTED, Lmax=4096, out_stride=1)
    refused("16", rc=_lib.LA_EUNSUPPORTED, top_k=17, top_stride=1)
    refused("65535", rc=_lib.LA_EUNSUPPORTED, batch=65536)


class _Stop(Exception):
    pass


def test_python_refusals_come_before_any_launch_and_the_training_entries_refuse_the_keyword(monkeypatch):
    from lyricalignment_amd import ops
    from lyricalignment_amd.finetune import FineTuner
    from lyricalignment_amd.harness import align_record_lines, align_record_lrc, align_song, suspect_characters
    from lyricalignment_amd.module.align_model import AlignModel
    ua = _ua()
    logits = torch.zeros((1, 20, 12))
    labels = torch.tensor([[3, 5, 7]])

    def launch(*a, **k):
        raise AssertionError("the refusal comes before anything is on a device")

    monkeypatch.setattr(ua, "_device_of", launch)
    monkeypatch.setattr(ops, "emissions_from_logits", launch)
    for f in (ua.perform_viterbi, ua.perform_viterbi_ctc):
        sig = inspect.signature(f).parameters
        assert list(sig)[-3:] == ["return_pronunciation", "pronunciation_classes", "pronunciation_top_k"]          # appended, with defaults
        assert sig["return_pronunciation"].default is False and sig["pronunciation_classes"].default is None
        assert sig["pronunciation_top_k"].default == 5
        with pytest.raises(ValueError, match="pronunciation_classes"):
            f(logits, labels, return_pronunciation=True)
        for top_k in (0, 17):
            with pytest.raises(ValueError, match="pronunciation_top_k"):
                f(logits, labels, return_pronunciation=True, pronunciation_classes=10, pronunciation_top_k=top_k)
        with pytest.raises(NotImplementedError, match="4095"):
            f(logits, labels, return_pronunciation=True, pronunciation_classes=4093)
        with pytest.raises(AssertionError):                             # good keywords are accepted (and go on to the device)
            f(logits, labels, return_pronunciation=True, pronunciation_classes=10)
    assert list(inspect.signature(ua._perform).parameters)[-3:] == ["return_pronunciation", "pronunciation_classes", "pronunciation_top_k"]
    assert list(inspect.signature(ua.align_labels).parameters)[-1] == "pron"

    class Unbuilt(AlignModel):                                          # align's keyword checks come before the engine exists
        def __init__(self):
            pass

        def engine(self):
            raise _Stop()

    audio = [np.zeros(16000, np.float32)]
    with pytest.raises(ValueError, match="pronunciation_classes"):
        AlignModel.align(Unbuilt(), audio, labels, return_pronunciation=True)
    with pytest.raises(ValueError, match="pronunciation_top_k"):
        AlignModel.align(Unbuilt(), audio, labels, return_pronunciation=True, pronunciation_classes=402, pronunciation_top_k=17)
    with pytest.raises(NotImplementedError):
        AlignModel.align(Unbuilt(), audio, labels, return_pronunciation=True, pronunciation_classes=4093)
    with pytest.raises(NotImplementedError):
        AlignModel.align(Unbuilt(), audio, labels, return_pronunciation=True, pronunciation_classes=4091, alternatives=[[(0, [9, 10])]])
    with pytest.raises(_Stop):
        AlignModel.align(Unbuilt(), audio, labels, return_pronunciation=True, pronunciation_classes=402)
    sig = inspect.signature(AlignModel.align).parameters
    assert list(sig)[-3:] == ["return_pronunciation", "pronunciation_classes", "pronunciation_top_k"]
    assert "return_pronunciation" in AlignModel.align.__doc__ and "pronunciation_classes" in AlignModel.align.__doc__

    with pytest.raises(ValueError, match="return_pronunciation"):
        ua.anchored_alignment_loss(logits, labels, return_pronunciation=True)
    with pytest.raises(ValueError, match="return_pronunciation"):
        FineTuner.micro_step_anchored(object(), audio, labels, return_pronunciation=True)

    for f in (align_record_lines, align_record_lrc, align_song):
        sig = inspect.signature(f).parameters
        assert sig["with_pronunciation"].default is False and sig["top_k"].default == 5
    assert inspect.signature(suspect_characters).parameters["min_gop"].default is None          # no threshold is built in
    assert inspect.signature(suspect_characters).parameters["max_rank"].default == 0


def test_the_harness_names_syllables_and_picks_the_suspects():
    from lyricalignment_amd.harness import PinyinClassLUT, _pronunciation_lines, _reading_kw, suspect_characters
    lut = PinyinClassLUT(["de", "le", "a"], {"sil": 0, "de": 3, "le": 5, "a": 7, "di": 4, "liao": 6, "d2": 3})
    assert lut.syllable_of(3) == "de" and lut.syllable_of(6) == "liao"   # the first syllable of the table for a class
    with pytest.raises(KeyError):
        lut.syllable_of(99)
    assert _reading_kw(lut, [[0]], None) == {} and _reading_kw(lut, [[0]], None).pronunciation is None
    kw = _reading_kw(lut, [[0, 1], [2]], None, True, 3)
    assert kw == {"return_pronunciation": True, "pronunciation_classes": [3, 4, 5, 6, 7], "pronunciation_top_k": 3}
    kw = _reading_kw(lut, [[0, 1], [2]], {0: ["di"]}, True, 2)
    assert kw["alternatives"] == [[(0, [4])]] and kw["return_readings"] is True and kw["pronunciation_top_k"] == 2
    clip = [{"class": 3, "frames": 4, "log_prob": -1.0, "rank": 0, "gop": 0.0, "top": [(3, -1.0), (4, -2.0)]}, None,
            {"class": 7, "frames": 2, "log_prob": -5.0, "rank": 3, "gop": -4.0, "top": [(6, -1.0), (5, -1.5)]}]
    result = _pronunciation_lines(clip, ["的了", "啊"], lut)
    assert result == [[{"char": "的", "class": 3, "syllable": "de", "frames": 4, "log_prob": -1.0, "rank": 0, "gop": 0.0,
                        "top": [("de", -1.0), ("di", -2.0)]}, None],
                      [{"char": "啊", "class": 7, "syllable": "a", "frames": 2, "log_prob": -5.0, "rank": 3, "gop": -4.0,
                        "top": [("liao", -1.0), ("le", -1.5)]}]]
    assert suspect_characters(result) == [(1, 0, "liao", -4.0)] == suspect_characters(result, max_rank=2)
    assert suspect_characters(result, max_rank=3) == [] and suspect_characters(result, max_rank=3, min_gop=-3.0) == [(1, 0, "liao", -4.0)]
    assert suspect_characters(result, max_rank=3, min_gop=-4.0) == []


def test_a_call_without_the_keyword_builds_exactly_the_rows_it_builds_today(monkeypatch):
    """align_labels on stubbed entries: off, the provider is asked once for the caller's own rows and ops.segment_class_scores is never
    called; on, it is asked once for the widened rows, the lattice reads a leading-column view of that matrix and the entry its trailing
    window."""
    from lyricalignment_amd import ops
    ua = _ua()
    lists = [[3, 5, 7], [9]]
    lab = torch.tensor([[3, 5, 7], [9, 0, 0]], dtype=torch.int32)
    n_lab = torch.tensor([3, 1], dtype=torch.int32)
    asked, scored, lattice = [], [], []

    def emissions_of(lab_x, n_x, needed=True):
        asked.append((lab_x.clone(), n_x.clone(), needed))
        return None, torch.zeros((2, 10, lab_x.shape[1] + 1))

    def run_lattice(em, lab_, n_, nf, *a, **k):
        lattice.append(em)
        on = torch.tensor([[0, 2, 4], [1, -1, -1]], dtype=torch.int32)
        return ua.LatticeResult(on, on + 2, torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.int32))

    def segment_class_scores(em_c, n_labels, onset, offset, own_col, top_k=5, want_scores=False, out=None):
        scored.append((em_c, own_col.clone(), top_k))
        B, L = onset.shape
        return (torch.zeros((B, L, top_k), dtype=torch.int32), torch.zeros((B, L, top_k), dtype=torch.float64),
                torch.zeros((B, L), dtype=torch.float64), torch.zeros((B, L), dtype=torch.int32), torch.ones((B, L), dtype=torch.int32))

    monkeypatch.setattr(ua, "run_lattice", run_lattice)
    monkeypatch.setattr(ops, "segment_class_scores", segment_class_scores)
    args = ("perform_viterbi", emissions_of, lab, n_lab, lists, [10, 10], 10, None, 0.02, None, 2, None, None, 0.0, None, None, 0.0, False,
            None, False)
    plain = ua.align_labels(*args)
    assert len(asked) == 1 and asked[0][0].tolist() == lab.tolist() and asked[0][1].tolist() == [3, 1] and not scored
    assert lattice[-1].shape == (2, 10, 4) and lattice[-1].is_contiguous()
    pron = ua._pronunciation_of("perform_viterbi", True, [1, 2], 2, lists)          # classes [1, 2, 3, 5, 7, 9]
    out = ua.align_labels(*args, pron=pron)
    assert len(asked) == 2 and asked[1][0].tolist() == [[3, 5, 7, 1, 2, 3, 5, 7, 9], [9, 1, 1, 1, 2, 3, 5, 7, 9]]
    assert asked[1][1].tolist() == [9, 9] and asked[1][2] is True
    assert lattice[-1].shape == (2, 10, 4) and lattice[-1].stride() == (100, 10, 1)          # the leading columns, through the row stride
    em_c, own_col, top_k = scored[0]
    assert len(scored) == 1 and em_c.shape == (2, 10, 6) and em_c.stride() == (100, 10, 1) and em_c.storage_offset() == 4 and top_k == 2
    assert em_c.untyped_storage().data_ptr() == lattice[-1].untyped_storage().data_ptr()       # no copy
    assert own_col.tolist() == [[2, 3, 4], [5, -1, -1]]
    assert isinstance(out, tuple) and len(out) == 2 and out[0] == plain
    assert [[d and d["class"] for d in row] for row in out[1]] == lists and out[1][0][0]["frames"] == 1
