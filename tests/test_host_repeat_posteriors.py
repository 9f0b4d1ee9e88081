"""CPU-only checks of the confidence for repeated lyric lines: the float64 yardstick tests/repeat_posterior_reference.py against exhaustive
path enumeration on small random lattices (repeat only, repeat + optional span, repeat + windows; one-label, nested and overlapping
spans), the visit identity, the yardstick without a repeat span against tests/window_posterior_reference.py, the host face of
la_alignment_posteriors_repeats (declared, exported, planner, argument checks answered before any device call) and the Python refusals
that need no device."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import repeat_posterior_reference as rpr
import window_posterior_reference as wpr
import windows_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LATTICES = 240
KEYS = ("gamma", "entry", "exit", "visits", "span_skip", "repeat_count")


def _random_lattice(i):
    """Lattice i of the family: i % 3 = 0 repeat only, 1 repeat + optional span, 2 repeat + windows.  L 1 .. 3, T 3 .. 7, soft
    emissions, up to two repeat spans (one-label, nested and overlapping ones occur), equal neighbour labels occur."""
    rs = np.random.RandomState(9000 + i)
    L = 1 + i % 3 if i < 30 else int(rs.randint(1, 4))
    T = int(rs.randint(max(3, L + 1), 8))
    labels = [int(v) for v in rs.randint(1, 4, size=L)]            # few classes: equal neighbours and equal span ends occur
    em = (-2.0 * rs.rand(T, L + 1)).astype(np.float32)
    rf = [-1] * L
    for _ in range(int(rs.randint(1, 3))):
        a = int(rs.randint(L))
        rf[a] = int(rs.randint(a + 1, L + 1))
    skip = lo = hi = None
    kind = i % 3
    if kind == 1:
        skip = [-1] * (L + 1)
        n = int(rs.randint(1, L + 1))
        skip[n] = int(rs.randint(n))
    if kind == 2:
        lo, hi = wr.open_windows(L, T)
        for s in rs.choice(2 * L + 1, size=int(rs.randint(1, 3)), replace=False):
            lo[s] = int(rs.randint(0, T // 2 + 1))
            hi[s] = int(rs.randint(lo[s] + 1, T + 1))
    return dict(em=em, labels=labels, skip=skip, pen=float(rs.choice([0.0, 0.5])), rf=rf, rpen=float(rs.choice([0.0, 0.5, 1.5])), lo=lo, hi=hi)


@functools.lru_cache(maxsize=None)
def _family():
    out = []
    for i in range(N_LATTICES):
        c = _random_lattice(i)
        args = (c["em"], c["labels"], c["skip"], c["pen"], c["rf"], c["rpen"], c["lo"], c["hi"])
        out.append((c, rpr.posteriors(*args), rpr.brute(*args)))
    return out


def test_the_family_holds_what_it_is_meant_to():
    fam = _family()
    assert len(fam) >= 200
    spans = [rpr.repeat_spans_of(c["rf"], len(c["labels"])) for c, _, _ in fam]
    assert sum(any(e == a + 1 for a, e in s) for s in spans) >= 10                                    # one-label spans
    assert sum(len(s) == 2 and s[0][0] < s[1][0] and s[1][1] <= s[0][1] for s in spans) >= 3          # nested
    assert sum(len(s) == 2 and s[0][0] < s[1][0] < s[0][1] < s[1][1] for s in spans) >= 1             # overlapping
    assert sum(len(s) == 2 and s[0][1] == s[1][1] for s in spans) >= 3                                # sharing an end
    assert sum(c["skip"] is not None for c, _, _ in fam) >= 60 and sum(c["lo"] is not None for c, _, _ in fam) >= 60
    assert sum(b is not None and b["repeat_count"].max() > 0.2 for _, _, b in fam) >= 50              # returns carry mass
    assert sum(b is not None and b["visits"].max() > 1.0 for _, _, b in fam) >= 20                    # counts above 1 occur
    assert sum(b is None for _, _, b in fam) >= 1                                                     # and windows without a path


def test_yardstick_equals_path_enumeration():
    worst = 0.0
    for i, (c, ref, bru) in enumerate(_family()):
        if bru is None:
            assert np.isneginf(ref["log_z"]) and all(not np.any(ref[k]) for k in KEYS), i
            continue
        assert abs(ref["log_z"] - bru["log_z"]) <= 1e-12, i
        for k in KEYS:
            d = float(np.max(np.abs(ref[k] - bru[k]))) if ref[k].size else 0.0
            worst = max(worst, d)
            assert d <= 1e-12, (i, k, d)
        assert np.allclose(ref["gamma"].sum(1), 1.0, atol=1e-12), i
    print("largest difference to enumeration", worst)


def test_the_visit_identity_holds_on_the_family():
    for i, (c, ref, bru) in enumerate(_family()):
        if bru is None:
            continue
        for r in (ref, bru):
            left, right = rpr.identity_sides(r["visits"], r["span_skip"], r["repeat_count"], c["skip"], c["rf"])
            assert np.max(np.abs(left - right)) <= 1e-12, (i, left, right)


@pytest.mark.parametrize("i", range(12))
def test_without_a_repeat_span_the_yardstick_is_the_window_posterior_reference(i):
    c = _random_lattice(60 + i)
    L, T = len(c["labels"]), c["em"].shape[0]
    lo, hi = (c["lo"], c["hi"]) if c["lo"] is not None else wr.open_windows(L, T)
    want = wpr.posteriors(c["em"], c["labels"], lo, hi, c["skip"], c["pen"])
    for rf in (None, [-1] * L):
        got = rpr.posteriors(c["em"], c["labels"], c["skip"], c["pen"], rf, 0.5, c["lo"], c["hi"])
        for k, w in zip(("gamma", "entry", "exit", "visits", "span_skip", "log_z"), want):
            assert np.allclose(got[k], w, rtol=0, atol=1e-13) or (np.isneginf(w) and np.isneginf(got[k])), (i, k)
        assert not got["repeat_count"].any()


def test_the_entry_points_are_declared_exported_and_check_arguments_on_the_host():
    from lyricalignment_amd import _lib
    text = open(os.path.join(ROOT, "include", "lyricalign.h")).read()
    assert "EXPECTED" in text and "visits[n]" in text and "repeat_count[a]" in text      # the expected-count semantics are stated
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("la_alignment_posteriors_repeats_workspace_bytes", "la_alignment_posteriors_repeats"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in lyricalign.h"
        assert name in _lib.SYMBOLS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} not exported"
    L = _lib.lib()
    who = "alignment_posteriors_repeats"
    need, need_win = ctypes.c_size_t(1), ctypes.c_size_t(2)
    f = L.la_alignment_posteriors_repeats_workspace_bytes
    for shape in ((32, 1500, 26), (2, 7000, 26), (3, 9000, 238), (1, 600, 511)):
        assert f(*shape, ctypes.byref(need)) == _lib.LA_OK
        assert L.la_alignment_posteriors_windows_workspace_bytes(*shape, ctypes.byref(need_win)) == _lib.LA_OK and need.value == need_win.value
    assert f(1, 600, 512, ctypes.byref(need)) == _lib.LA_EUNSUPPORTED and "511" in _lib.last_error()
    assert f(1, 600, 26, None) == _lib.LA_EINVAL

    P = 16                                      # a non-null, aligned stand-in pointer: every call below is refused before any device call
    big = 1 << 40

    def call(em=P, labels=P, n_labels=P, n_frames=P, batch=2, T=100, Lmax=26, onset=P, offset=P, out_stride=26, bw=2, skip_from=P,
             skip_stride=27, penalty=0.0, win_lo=P, win_hi=P, win_stride=53, repeat_from=P, repeat_stride=26, repeat_penalty=0.0, path=P,
             path_stride=100, occupancy=P, onset_prob=P, offset_prob=P, visits=P, span_skip_prob=P, repeat_count=P, path_prob=P, log_z=P,
             status=P, gamma=0, gamma_bs=0, gamma_rs=0, ws=P, ws_bytes=big, em_rs=27, labels_stride=26):
        return L.la_alignment_posteriors_repeats(em, T * em_rs, em_rs, labels, labels_stride, n_labels, n_frames, batch, T, Lmax, onset, offset,
                                                 out_stride, bw, skip_from, skip_stride, penalty, win_lo, win_hi, win_stride, repeat_from,
                                                 repeat_stride, repeat_penalty, path, path_stride, occupancy, onset_prob, offset_prob, visits,
                                                 span_skip_prob, repeat_count, path_prob, log_z, status, gamma, gamma_bs, gamma_rs, ws, ws_bytes, 0)

    for null in ("em", "labels", "n_labels", "n_frames", "onset", "offset", "occupancy", "onset_prob", "offset_prob", "visits",
                 "span_skip_prob", "repeat_count", "log_z", "status"):
        assert call(**{null: 0}) == _lib.LA_EINVAL, null
        assert "null" in _lib.last_error() and who in _lib.last_error(), null
    assert call(win_lo=0) == _lib.LA_EINVAL and "go together" in _lib.last_error()
    assert call(win_hi=0) == _lib.LA_EINVAL and "go together" in _lib.last_error()
    assert call(win_stride=52) == _lib.LA_EINVAL and "strides" in _lib.last_error()
    assert call(skip_stride=26) == _lib.LA_EINVAL and "strides" in _lib.last_error()
    assert call(penalty=-0.5) == _lib.LA_EINVAL and "skip_penalty" in _lib.last_error()
    assert call(bw=-1) == _lib.LA_EINVAL and "boundary_window" in _lib.last_error()
    assert call(repeat_penalty=-0.5) == _lib.LA_EINVAL and "repeat_penalty" in _lib.last_error()
    assert call(repeat_penalty=float("nan")) == _lib.LA_EINVAL and "repeat_penalty" in _lib.last_error()
    assert call(repeat_stride=25) == _lib.LA_EINVAL and "repeat_stride" in _lib.last_error() and who in _lib.last_error()
    assert call(path_stride=99) == _lib.LA_EINVAL and "path_stride" in _lib.last_error()
    assert call(path=0, path_stride=99, path_prob=P) == _lib.LA_EINVAL                      # path_prob without path
    assert call(path=0) == _lib.LA_EINVAL and "path_prob" in _lib.last_error()
    assert call(path_prob=0, path_stride=99) == _lib.LA_EINVAL and "path_stride" in _lib.last_error()   # a path alone is checked too
    assert call(gamma=P, gamma_bs=100 * 53, gamma_rs=52) == _lib.LA_EINVAL and "gamma" in _lib.last_error()
    assert call(out_stride=25) == _lib.LA_EINVAL
    assert call(em_rs=26) == _lib.LA_EINVAL
    assert call(T=0) == _lib.LA_EINVAL
    assert call(Lmax=512, out_stride=512, em_rs=513, labels_stride=512, skip_stride=513, win_stride=1025, repeat_stride=512) == _lib.LA_EUNSUPPORTED
    assert "511" in _lib.last_error() and who in _lib.last_error()
    assert call(ws_bytes=2 * 100 * 64 * 8 - 1) == _lib.LA_EINVAL and "workspace too small" in _lib.last_error()
    assert call(ws=0) == _lib.LA_EINVAL
    assert call(batch=0) == _lib.LA_OK          # nothing to do, nothing enqueued
    # the optional inputs may each be absent: refused only further on (here: by the missing workspace)
    assert call(skip_from=0, win_lo=0, win_hi=0, repeat_from=0, path=0, path_prob=0, repeat_stride=0, path_stride=0, win_stride=0, ws=0) == _lib.LA_EINVAL
    assert "workspace" in _lib.last_error()


def test_python_refusals_that_need_no_device():
    import torch
    from lyricalignment_amd.harness import align_record_lines
    from lyricalignment_amd.utils import alignment as ua
    rows = torch.zeros((1, 6), dtype=torch.int32)
    for kind in ("plain", "span", "anchored", "sheet"):                 # the four older kinds keep refusing the repeat lattice
        with pytest.raises(ValueError):
            ua.run_lattice(*[None] * 4, confidence=kind, repeat_from=rows)
    with pytest.raises(ValueError):
        ua.run_lattice(*[None] * 4, confidence="visits")
    wide = torch.zeros((1, 512), dtype=torch.int32)
    with pytest.raises(NotImplementedError):                            # before anything is launched: no tensor is on a device
        ua.run_lattice(None, wide, None, None, confidence="repeat", repeat_from=torch.full((1, 512), -1, dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        ua.run_lattice(None, wide, None, None, confidence="repeat")
    for name in ("perform_viterbi_repeat_scored", "perform_viterbi_ctc_repeat_scored", "_formatted_repeat"):
        assert callable(getattr(ua, name))
    r = ua._result((1, 2, 3, 4, 5))                                     # the DP alone: eleven fields, seven None, the path behind them
    assert isinstance(r, ua.RepeatLatticeResult) and isinstance(r, ua.LatticeResult)
    assert len(r) == 11 and list(r[4:]) == [None] * 7 and r.path == 5 and r.repeat_count is None and r.path_prob is None
    r = ua._result((1, 2, 3, 4, 5), (6, 7, 8, 9, "status", 10, 11, 12, 13))      # the repeat sweep's nine outputs behind the DP's five
    assert isinstance(r, ua.RepeatLatticeResult) and list(r[4:8]) == [6, 7, 8, 9] and r.log_z_free is None
    assert len(r) == 11 and r.present_prob == 10 and r.visits == 10 and r.span_skip_prob == 11 and (r.repeat_count, r.path_prob) == (12, 13)
    r = ua._result((1, 2, 3, 4))                                        # no path: a LatticeResult, the four attributes readable and None
    assert type(r) is ua.LatticeResult and (r.path, r.visits, r.repeat_count, r.path_prob) == (None,) * 4
    assert ua._visits_of_row([0, 1, 1, 2, 3, 3, 1, 1, 4, -1]) == [(0, 1, 3), (1, 4, 6), (0, 6, 8)]
    import inspect
    assert "with_visit_confidence" in inspect.signature(align_record_lines).parameters
    from lyricalignment_amd.module.align_model import AlignModel
    assert "return_repeat_confidence" in inspect.signature(AlignModel.align).parameters
