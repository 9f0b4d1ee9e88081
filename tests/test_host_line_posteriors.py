"""CPU-only checks of the confidence for free line order: the all-pairs float64 yardstick (tests/line_posterior_reference.py) against
exhaustive path enumeration, its identities (visits constant along a line, gamma rows sum to 1, penalty +inf = the plain lattice's
posteriors, one line = the repeat lattice's with the whole sheet repeatable), the routing of confidence="lines" with the device calls
stubbed, every refusal before a device is asked for, keyword positions and defaults, the harness function, and the host face of
la_alignment_posteriors_lines (declared, exported, argument checks answered before any device call)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import line_order_reference as lo
import line_posterior_reference as lp
import posterior_reference as pr
import repeat_posterior_reference as rpr
from conftest import ROOT

KEYS = ("gamma", "entry", "exit", "visits", "in_order", "log_z")


def _tiny(rs):
    n_lines = int(rs.randint(1, 5))
    lengths = [int(rs.randint(1, 3)) for _ in range(n_lines)]
    L, T = sum(lengths), int(rs.randint(2, 7))
    labels = [int(v) for v in rs.randint(1, 3, size=L)]                            # two classes: they collide across line ends and starts
    em = np.log(rs.dirichlet(np.ones(L + 1), size=T)).astype(np.float32)
    return em, labels, lo.flags_of_lengths(lengths), lengths


# ------------------------------------------------------------------------------------------------ 1. exhaustive enumeration
def test_the_yardstick_equals_exhaustive_enumeration():
    """1 .. 4 lines of 1 .. 2 labels over a two-class alphabet, 2 .. 6 frames, penalties 0 / 0.7 / 2 / +inf: gamma, entry, exit, visits,
    in_order and log_z of the log-domain forward-backward equal the sums over ALL lattice paths; some of the lattices have no path."""
    rs = np.random.RandomState(0)
    seen, infeasible, collide, worst = set(), 0, 0, 0.0
    for case in range(60):
        em, labels, ls, lengths = _tiny(rs)
        starts = lo.line_starts_of(ls, len(labels))
        collide += any(labels[a] == labels[e - 1] for a in starts for e in starts[1:] + [len(labels)])
        for pen in (0.0, 0.7, 2.0, float("inf")):
            got, want = lp.posteriors(em, labels, ls, pen), lp.brute(em, labels, ls, pen)
            if np.isneginf(want["log_z"]):
                infeasible += 1
                assert np.isneginf(got["log_z"]) and not got["gamma"].any() and not got["visits"].any(), (case, pen)
                continue
            seen.add((len(lengths), pen))
            for k in KEYS:
                d = float(np.abs(np.asarray(got[k]) - np.asarray(want[k])).max())
                worst = max(worst, d)
                assert d <= 1e-12 * max(1.0, float(np.abs(np.asarray(want[k])).max())), (case, pen, k, d)
    assert {n for n, _ in seen} == {1, 2, 3, 4} and {p for _, p in seen} == {0.0, 0.7, 2.0, float("inf")}
    assert infeasible > 0 and collide > 20, (infeasible, collide)


# ------------------------------------------------------------------------------------------------ 2. identities
def test_identities_of_the_yardstick():
    rs = np.random.RandomState(4)
    multi = 0
    for case in range(30):
        L, T = int(rs.randint(2, 10)), int(rs.randint(12, 40))
        labels = [int(v) for v in rs.randint(1, 4, size=L)]
        em = np.log(rs.dirichlet(np.ones(L + 1), size=T)).astype(np.float32)
        starts = [0] + sorted(rs.choice(np.arange(1, L), size=int(rs.randint(0, L)), replace=False).tolist())
        ls = [1 if n in starts else 0 for n in range(L)]
        pen = (0.0, 0.3, 2.0)[case % 3]
        r = lp.posteriors(em, labels, ls, pen)
        assert np.allclose(r["gamma"].sum(1), 1.0, rtol=0, atol=1e-12)
        for a, e in zip(starts, starts[1:] + [L]):                                 # a line is entered at its start and left at its end
            assert np.allclose(r["visits"][a:e], r["visits"][a], rtol=0, atol=1e-12), (case, a, e)
        assert np.allclose(r["entry"].sum(0), r["exit"].sum(0), rtol=0, atol=1e-12)
        assert (r["in_order"] <= r["visits"] + 1e-12).all() and not r["in_order"][[n for n in range(L) if n not in starts]].any()
        multi += (r["visits"] > 1.2).any()
        # a prohibitive penalty: the plain lattice
        if T >= 2 * L:
            inf = lp.posteriors(em, labels, ls, float("inf"))
            gamma, entry, exit_, log_z = pr.posteriors(em, labels)
            assert abs(inf["log_z"] - log_z) <= 1e-12 * max(1.0, abs(log_z))
            for k, w in (("gamma", gamma), ("entry", entry), ("exit", exit_)):
                assert np.allclose(inf[k], w, rtol=0, atol=1e-12), (case, k)
            assert np.allclose(inf["visits"], 1.0, rtol=0, atol=1e-12) and np.allclose(inf["in_order"], ls, rtol=0, atol=1e-12)
        # one line: the whole sheet repeatable, the same penalty
        one = lp.posteriors(em, labels, [1] + [0] * (L - 1), pen)
        rep = rpr.posteriors(em, labels, repeat_from=[L] + [-1] * (L - 1), repeat_penalty=pen)
        assert abs(one["log_z"] - rep["log_z"]) <= 1e-12 * max(1.0, abs(rep["log_z"]))
        for k in ("gamma", "entry", "exit", "visits"):
            assert np.allclose(one[k], rep[k], rtol=0, atol=1e-12), (case, k)
        assert abs((one["visits"][0] - one["in_order"][0]) - rep["repeat_count"][0]) <= 1e-12     # out of print order = the returns
    assert multi > 5


def test_log_z_only_is_the_forward_sweep():
    rs = np.random.RandomState(2)
    em, labels, ls, _ = _tiny(rs)
    assert lp.log_z_only(em, labels, ls, 0.7) == lp.posteriors(em, labels, ls, 0.7)["log_z"]


# ------------------------------------------------------------------------------------------------ 3. routing and refusals, the device stubbed
class _Stop(Exception):
    pass


def test_run_lattice_routes_the_line_confidence_to_the_dp_and_then_the_new_sweep(monkeypatch):
    from lyricalignment_amd import ops
    from lyricalignment_amd.utils import alignment as ua
    seen = []
    z = torch.zeros((1, 3), dtype=torch.int32)
    path = torch.ones((1, 5), dtype=torch.int32)

    def dp(em, lab, n_lab, nf, line_start, line_jump_penalty=0.0):
        seen.append(("dp", line_start.tolist(), line_jump_penalty))
        return z, z + 1, torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int32), path

    def sweep(em, lab, n_lab, nf, onset, offset, line_start, line_jump_penalty=0.0, path=None, boundary_window=2, want_gamma=False):
        seen.append(("sweep", onset is z, line_start.tolist(), line_jump_penalty, path.tolist(), boundary_window))
        f = torch.arange(3, dtype=torch.float32)[None]
        return f, f + 1, f + 2, torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int32), f + 3, f + 4, torch.ones((1, 5))

    for name in dir(ops):
        if name.startswith(("viterbi_", "alignment_posteriors")):
            monkeypatch.setattr(ops, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("another entry was launched")))
    monkeypatch.setattr(ops, "viterbi_lines_batch", dp)
    monkeypatch.setattr(ops, "alignment_posteriors_lines", sweep)
    em, lab = torch.zeros((1, 5, 4)), torch.tensor([[3, 5, 7]], dtype=torch.int32)
    n_lab, nf = torch.tensor([3], dtype=torch.int32), torch.tensor([5], dtype=torch.int32)
    ls = torch.tensor([[1, 0, 1]], dtype=torch.int32)
    r = ua.run_lattice(em, lab, n_lab, nf, confidence="lines", boundary_window=3, line_start=ls, line_jump_penalty=0.75)
    assert seen == [("dp", [[1, 0, 1]], 0.75), ("sweep", True, [[1, 0, 1]], 0.75, [[1] * 5], 3)]
    assert isinstance(r, ua.RepeatLatticeResult) and r.path is path
    assert r.occupancy.tolist() == [[0, 1, 2]] and r.offset_prob.tolist() == [[2, 3, 4]] and r.log_z.tolist() == [1.0]
    assert r.visits.tolist() == [[3, 4, 5]] and r.present_prob is r.visits and r.in_order.tolist() == [[4, 5, 6]]
    assert r.path_prob.shape == (1, 5) and r.span_skip_prob is None and r.log_z_free is None
    # without the kind: the DP alone, as before
    del seen[:]
    r = ua.run_lattice(em, lab, n_lab, nf, line_start=ls, line_jump_penalty=0.75)
    assert [s[0] for s in seen] == ["dp"] and r.occupancy is None and r.in_order is None
    # the six older kinds keep raising with a line_start; "lines" needs one
    for kind in ("plain", "span", "anchored", "sheet", "repeat", "song"):
        with pytest.raises(ValueError, match="line_start"):
            ua.run_lattice(em, lab, n_lab, nf, line_start=ls, confidence=kind)
    with pytest.raises(ValueError, match="line_start"):
        ua.run_lattice(em, lab, n_lab, nf, confidence="lines")
    skip = torch.full((1, 4), -1, dtype=torch.int32)
    with pytest.raises(ValueError, match="line_start"):
        ua.run_lattice(em, lab, n_lab, nf, line_start=ls, confidence="lines", skip_from=skip)
    assert len(seen) == 1
    assert ua.LINES_SWEEP == "alignment_posteriors_lines" and len(ua.ROUTES) == 28 and not any(k[0] == "lines" for k in ua.ROUTES)
    names = list(inspect.signature(ua.run_lattice).parameters)
    assert names[-2:] == ["line_start", "line_jump_penalty"] and len(names) == 14


CONFIDENCES = ("return_confidence", "return_span_confidence", "return_anchored_confidence", "return_sheet_confidence",
               "return_repeat_confidence", "return_song_confidence")


def test_every_refusal_comes_before_a_device_is_asked_for(monkeypatch):
    from lyricalignment_amd import ops
    from lyricalignment_amd.module.align_model import AlignModel
    from lyricalignment_amd.utils import alignment as ua
    logits = torch.zeros((1, 20, 12))
    labels = torch.tensor([[3, 5, 7]])

    def launch(*a, **k):
        raise _Stop()

    monkeypatch.setattr(ua, "_device_of", launch)
    for name in ("emissions_from_logits", "viterbi_lines_batch", "alignment_posteriors_lines"):
        monkeypatch.setattr(ops, name, launch)

    class Unbuilt(AlignModel):                                          # align's keyword checks come before the engine exists
        def __init__(self):
            pass

        def engine(self):
            raise _Stop()

    audio = [np.zeros(16000, np.float32)]
    align = lambda **kw: AlignModel.align(Unbuilt(), audio, labels, **kw)
    with pytest.raises(ValueError, match="return_line_confidence.*line_starts"):
        align(return_line_confidence=True)
    with pytest.raises(ValueError, match="return_line_confidence.*line_starts"):
        align(return_line_confidence=True, optional_spans=[[(0, 1)]])
    for name in CONFIDENCES:                                            # the six older keywords keep raising next to line_starts
        for more in ({}, {"return_line_confidence": True}):
            with pytest.raises(ValueError, match=rf"line_starts.*{name}"):
                align(line_starts=[[0, 2]], **{name: True}, **more)
    for bad in ([[1]], [[0, 0]], [[0, 3]], [[]]):
        with pytest.raises(ValueError, match="line_starts"):
            align(line_starts=bad, return_line_confidence=True)
    for pen in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="line_jump_penalty"):
            align(line_starts=[[0, 2]], line_jump_penalty=pen, return_line_confidence=True)
    for name, value in dict(optional_spans=[[(0, 1)]], repeat_spans=[[(0, 2)]], onset_anchors=[[(0, 0.1, 0.1)]], off_sheet=[[1]]).items():
        with pytest.raises(ValueError, match=rf"line_starts.*{name}"):
            align(line_starts=[[0, 2]], return_line_confidence=True, **{name: value})
    with pytest.raises(_Stop):                                          # good keywords go on to the device
        align(line_starts=[[0, 2]], line_jump_penalty=0.5, return_line_confidence=True, return_segments=True)
    for two in (ua.perform_viterbi_line_confidence, ua.perform_viterbi_ctc_line_confidence):
        with pytest.raises(ValueError, match="line_starts"):
            two(logits, labels, None)
        with pytest.raises(ValueError, match="line_starts"):
            two(logits, labels, [[0, 3]])
        for pen in (-1.0, float("nan")):
            with pytest.raises(ValueError, match="line_jump_penalty"):
                two(logits, labels, [[0, 2]], pen)
        with pytest.raises(NotImplementedError, match="4095"):
            two(torch.zeros((1, 4, 12)), [list(np.arange(4096) % 11 + 1)], [[0]])
        with pytest.raises(_Stop):
            two(logits, labels, [[0, 2]], 0.5)


# ------------------------------------------------------------------------------------------------ 4. keyword positions and defaults
def test_keyword_positions_and_defaults():
    from lyricalignment_amd import ops
    from lyricalignment_amd.harness import align_free_order, align_free_order_scored
    from lyricalignment_amd.module.align_model import AlignModel
    from lyricalignment_amd.utils import alignment as ua
    sig = inspect.signature(AlignModel.align).parameters
    names = list(sig)
    i = names.index("return_off_sheet")
    assert names[i + 1] == "return_line_confidence" and names[i + 2] == "return_pronunciation"           # directly after return_off_sheet
    assert sig["return_line_confidence"].default is False and sig["return_line_confidence"].kind is inspect.Parameter.KEYWORD_ONLY
    assert names[-3:] == ["return_pronunciation", "pronunciation_classes", "pronunciation_top_k"]
    for f in (ua.perform_viterbi_line_confidence, ua.perform_viterbi_ctc_line_confidence):
        sig = inspect.signature(f).parameters
        assert list(sig)[:5] == ["prediction", "labels", "line_starts", "line_jump_penalty", "boundary_window"], f.__name__
        assert sig["line_starts"].default is inspect.Parameter.empty and sig["line_jump_penalty"].default == 0.0
        assert sig["boundary_window"].default == 2 and not f.__name__.endswith("_scored")
    for f in (ua.perform_viterbi, ua.perform_viterbi_ctc, ua._perform):                                  # the older functions keep their lists
        assert "return_line_confidence" not in inspect.signature(f).parameters
    assert list(inspect.signature(ops.alignment_posteriors_lines).parameters) == [
        "em", "labels", "n_labels", "n_frames", "onset", "offset", "line_start", "line_jump_penalty", "path", "boundary_window", "want_gamma"]
    sig = inspect.signature(ops.alignment_posteriors_lines).parameters
    assert sig["line_jump_penalty"].default == 0.0 and sig["path"].default is None and sig["boundary_window"].default == 2
    assert "alignment_posteriors_lines" not in ops._ENTRIES and len(ops._ENTRIES) == 11                  # a wrapper of its own
    assert list(inspect.signature(align_free_order_scored).parameters) == list(inspect.signature(align_free_order).parameters) + ["boundary_window"]
    sig = inspect.signature(align_free_order_scored).parameters
    assert sig["use_ctc_loss"].default is True and sig["line_jump_penalty"].default == 0.0 and sig["heteronyms"].default is None
    assert sig["boundary_window"].default == 2
    for doc in (ua.perform_viterbi_line_confidence.__doc__, align_free_order_scored.__doc__):
        assert "not been tuned on real singing" in " ".join(doc.lower().split())
    assert "not a probability" in " ".join(align_free_order_scored.__doc__.lower().split())


# ------------------------------------------------------------------------------------------------ 5. the harness
def test_align_free_order_scored_from_a_stubbed_align():
    from lyricalignment_amd.harness import PinyinClassLUT, align_free_order, align_free_order_scored
    lines = ["ab", "cde", "f", "gh"]
    seen = {}
    # sung: line 1, line 0, line 1, line 2, line 1 (line 3 never); every visit 0.05 s, except the last one of 0.15 s
    sung = [2, 3, 4, 0, 1, 2, 3, 4, 5, 2, 3, 4]
    segments = [[(n, 0.1 * i, 0.1 * i + (0.15 if i == 11 else 0.05)) for i, n in enumerate(sung)]]
    seconds = [[[0.3, 0.35], [0.4, 0.45], [0.0, 0.05], [0.1, 0.15], [0.2, 0.25], [0.8, 0.85], None, None]]
    occupancy = [0.9, 0.8, 0.7, 1.0, 0.5, 0.6, 0.6, 0.6, 0.25, 1.0, 1.0, 0.2]
    scores = [{"occupancy": [0.0] * 8, "onset_prob": [0.0] * 8, "offset_prob": [0.0] * 8, "path_log_posterior": -1.25, "visits": [0.0] * 8,
               "visit_occupancy": occupancy, "line_visits": [1.0, 2.75, 0.5, 0.0], "line_out_of_order": [1.0, 2.5, 0.0, 0.0]}]

    class Model:
        def align(self, audios, labels, **kw):
            seen.update(kw, n_audio=len(audios))
            return (seconds, segments, scores) if kw.get("return_line_confidence") else (seconds, segments)

    lut = PinyinClassLUT(["a", "b", "c", "d", "e", "f", "g", "h"], {c: i + 1 for i, c in enumerate("abcdefgh")})
    tok = lambda line: ["abcdefgh".index(c) for c in line]
    out = align_free_order_scored(Model(), np.zeros(1600, np.float32), lines, lut, tok, line_jump_penalty=0.5, boundary_window=3)
    assert seen["line_starts"] == [[0, 2, 5, 6]] and seen["line_jump_penalty"] == 0.5 and seen["return_segments"] is True
    assert seen["return_line_confidence"] is True and seen["boundary_window"] == 3 and seen["use_ctc"] is True
    seen.clear()
    plain = align_free_order(Model(), np.zeros(1600, np.float32), lines, lut, tok, line_jump_penalty=0.5)
    assert "return_line_confidence" not in seen and "boundary_window" not in seen                       # the call as it was
    assert set(out) == set(plain) | {"confidence"} and all(out[k] == plain[k] for k in plain)
    assert out["order"] == [1, 0, 1, 2, 1] and out["unsung"] == [3]
    conf = out["confidence"]
    assert set(conf) == {"expected_occurrences", "out_of_order", "occurrence_occupancy", "order_log_posterior"}
    assert conf["expected_occurrences"] == [1.0, 2.75, 0.5, 0.0] and conf["out_of_order"] == [1.0, 2.5, 0.0, 0.0]
    assert conf["order_log_posterior"] == -1.25
    occ = conf["occurrence_occupancy"]
    assert [len(o) for o in occ] == [1, 3, 1, 0]
    assert occ[0] == [pytest.approx(0.75)] and occ[2] == [pytest.approx(0.25)]
    assert occ[1][:2] == [pytest.approx(0.8), pytest.approx(0.6)]
    assert occ[1][2] == pytest.approx((1.0 * 0.05 + 1.0 * 0.05 + 0.2 * 0.15) / 0.25)                    # weighted by the visits' frames
    with pytest.raises(ValueError, match="align_free_order_scored"):
        align_free_order_scored(Model(), np.zeros(1600, np.float32), lines, lut, lambda line: [0])


# ------------------------------------------------------------------------------------------------ 6. the library's host face
def test_the_entry_points_are_declared_exported_and_check_arguments_on_the_host():
    from lyricalignment_amd import _lib
    text = open(os.path.join(ROOT, "include", "lyricalign.h")).read()
    assert "No posteriors and no training loss exist on this lattice" not in " ".join(text.split())
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    C = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
    for name in ("la_alignment_posteriors_lines_workspace_bytes", "la_alignment_posteriors_lines"):
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert decl, f"{name} not declared in lyricalign.h"
        assert name in _lib.SYMBOLS and _lib.SYMBOLS[name][0] is ctypes.c_int32
        args = [a.strip() for a in decl.group(1).split(",")]
        assert len(args) == len(_lib.SYMBOLS[name][1]), name
        for a, ctype in zip(args, _lib.SYMBOLS[name][1]):                # argument by argument
            if "*" in a:
                assert ctype in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)), (name, a)
            else:
                assert ctype is C[a.split()[-2]], (name, a)
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} not exported"
    arg_names = lambda n: [a.strip().split()[-1].lstrip("*") for a in re.search(r"\bint\s+" + n + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")]
    plain = arg_names("la_alignment_posteriors")
    assert arg_names("la_alignment_posteriors_lines") == (
        plain[:14] + ["line_start", "line_stride", "line_jump_penalty", "path", "path_stride"] + plain[14:17]
        + ["visits", "in_order", "path_prob"] + plain[17:])

    L = _lib.lib()
    need = ctypes.c_size_t(1)
    f = L.la_alignment_posteriors_lines_workspace_bytes
    # every alpha row, the jump term of every label position and three sums per label position, float64
    for shape, states in (((32, 1500, 26), 64), ((2, 7000, 40), 128), ((3, 900, 238), 512), ((1, 600, 511), 1024), ((1, 600, 512), 2048),
                          ((1, 1200, 2500), 8192), ((2, 50, 4095), 8192)):
        assert f(*shape, ctypes.byref(need)) == _lib.LA_OK
        assert need.value == shape[0] * (shape[1] * (states + states // 2) + 3 * (states // 2)) * 8, shape
    assert f(1, 600, 4096, ctypes.byref(need)) == _lib.LA_EUNSUPPORTED and "4095" in _lib.last_error()
    assert f(1, 600, 26, None) == _lib.LA_EINVAL

    P = 16                                      # a non-null, aligned stand-in pointer: every call below is refused before any device call
    big = 1 << 40

    def call(em=P, labels=P, n_labels=P, n_frames=P, batch=2, T=100, Lmax=26, onset=P, offset=P, out_stride=26, window=2, line_start=P,
             line_stride=26, penalty=0.0, path=P, path_stride=100, occupancy=P, onset_prob=P, offset_prob=P, visits=P, in_order=P, path_prob=P,
             log_z=P, status=P, gamma=0, gamma_bs=0, gamma_rs=0, ws=P, ws_bytes=big, em_rs=27, labels_stride=26):
        return L.la_alignment_posteriors_lines(em, T * em_rs, em_rs, labels, labels_stride, n_labels, n_frames, batch, T, Lmax, onset, offset,
                                               out_stride, window, line_start, line_stride, penalty, path, path_stride, occupancy, onset_prob,
                                               offset_prob, visits, in_order, path_prob, log_z, status, gamma, gamma_bs, gamma_rs, ws, ws_bytes, 0)

    who = "alignment_posteriors_lines"
    for null in ("em", "labels", "n_labels", "n_frames", "onset", "offset", "line_start", "occupancy", "onset_prob", "offset_prob", "visits",
                 "in_order", "log_z", "status"):
        assert call(**{null: 0}) == _lib.LA_EINVAL, null
        assert "null" in _lib.last_error() and who in _lib.last_error()
    for pen in (-0.5, float("nan"), float("-inf")):
        assert call(penalty=pen) == _lib.LA_EINVAL and "line_jump_penalty" in _lib.last_error()
    assert call(window=-1) == _lib.LA_EINVAL and "boundary_window" in _lib.last_error()
    assert call(path=0) == _lib.LA_EINVAL and "path_prob" in _lib.last_error()              # path_prob without the path
    assert call(line_stride=25) == _lib.LA_EINVAL and "strides" in _lib.last_error()
    assert call(out_stride=25) == _lib.LA_EINVAL and call(em_rs=26) == _lib.LA_EINVAL and call(labels_stride=25) == _lib.LA_EINVAL
    assert call(path_stride=99) == _lib.LA_EINVAL and "path_stride" in _lib.last_error()
    assert call(gamma=P, gamma_bs=100 * 53, gamma_rs=52) == _lib.LA_EINVAL and "gamma" in _lib.last_error()
    assert call(gamma=P, gamma_bs=100 * 53 - 1, gamma_rs=53) == _lib.LA_EINVAL
    assert call(T=0) == _lib.LA_EINVAL and call(batch=-1) == _lib.LA_EINVAL
    assert call(Lmax=4096, out_stride=4096, em_rs=4097, labels_stride=4096, line_stride=4096) == _lib.LA_EUNSUPPORTED
    assert "4095" in _lib.last_error() and who in _lib.last_error()
    assert call(ws_bytes=2 * (100 * 96 + 96) * 8 - 1) == _lib.LA_EINVAL and "workspace too small" in _lib.last_error()
    assert call(ws=0) == _lib.LA_EINVAL
    assert call(ws=P + 4) == _lib.LA_EINVAL and "aligned" in _lib.last_error()
    assert call(batch=0) == _lib.LA_OK          # nothing to do, nothing enqueued
