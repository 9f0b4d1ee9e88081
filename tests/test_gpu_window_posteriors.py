"""la_alignment_posteriors_windows (the WIN instantiations of csrc/la_posterior.hip) on the GPU against the float64 numpy yardstick
tests/window_posterior_reference.py (pinned to brute-force enumeration by tests/test_host_window_posteriors.py, which also asserts that
the window sets used here have a path and move gamma by more than 0.5), against la_alignment_posteriors_spans / la_alignment_posteriors
with all-open windows, the window edges, one ragged launch, and the Python surface that carries the anchored confidences (ops,
AlignModel.align, utils.alignment, harness) on the tiny random-weight model of tests/test_gpu_ragged.py.

Tolerance: absolute 8 * T * 2**-23 on every probability and on log_z, derived in tests/test_gpu_span_posteriors.py (T steps of alpha and
of beta with a float32 log-sum-exp correction of <= ~2**-23 each, gamma adds the two, a two-fold margin for hardware exp / log).  It
carries over unchanged: a gated cell is exactly -inf and adds no rounding.  window_log_prob is a difference of two such log_z values:
16 * T * 2**-23.

Two cases of the issue's list cannot be LA_OK in any implementation and are kept as agreement on LA_EINFEASIBLE instead of being dropped:
the span-free lattice of 511 labels in 300 frames (the span-free lattice of 511 labels is checked at 600 frames, an added shape), and
T = 1 at L = 2 among the prefetch edges (start states 0 / 1, end states 3 / 4), as in tests/test_gpu_windows.py.
"""
import json

import numpy as np
import pytest
import torch

import span_posterior_reference as spr
import window_posterior_reference as wpr
import windows_reference as wr
from conftest import e2e_cases

pytestmark = pytest.mark.gpu

HOP = 0.02
SHARED = ("occupancy", "onset_prob", "offset_prob", "log_z", "status")
NAMES = SHARED + ("present_prob", "span_skip_prob")
PROBS = ("occupancy", "onset_prob", "offset_prob", "present_prob", "span_skip_prob")


def _tol(T):
    return 8 * T * 2.0 ** -23


def _pack(ems, labels_list, skips, los, his, Tmax=None, Lmax=None, T_list=None):
    """skips None: a null skip_from.  Window rows are padded with the closed window [0, 0)."""
    B = len(ems)
    Lmax = Lmax or max(max(len(l) for l in labels_list), 1)
    Tmax = Tmax or max(e.shape[0] for e in ems)
    em = torch.zeros((B, Tmax, Lmax + 1), dtype=torch.float32)
    labels = torch.zeros((B, Lmax), dtype=torch.int32)
    skip = torch.full((B, Lmax + 1), -1, dtype=torch.int32)
    lo = torch.zeros((B, 2 * Lmax + 1), dtype=torch.int32)
    hi = torch.zeros((B, 2 * Lmax + 1), dtype=torch.int32)
    for b, (e, l) in enumerate(zip(ems, labels_list)):
        em[b, : e.shape[0], : e.shape[1]] = torch.from_numpy(np.ascontiguousarray(e))
        labels[b, : len(l)] = torch.tensor(list(l), dtype=torch.int32)
        if skips is not None:
            skip[b, : len(skips[b])] = torch.tensor(list(skips[b]), dtype=torch.int32)
        lo[b, : len(los[b])] = torch.tensor(list(los[b]), dtype=torch.int32)
        hi[b, : len(his[b])] = torch.tensor(list(his[b]), dtype=torch.int32)
    n_labels = torch.tensor([len(l) for l in labels_list], dtype=torch.int32)
    n_frames = torch.tensor([e.shape[0] for e in ems] if T_list is None else T_list, dtype=torch.int32)
    return em.cuda(), labels.cuda(), n_labels.cuda(), n_frames.cuda(), None if skips is None else skip.cuda(), lo.cuda(), hi.cuda()


def _launch(ems, labels_list, skips, penalty, los, his, window=2, Tmax=None, Lmax=None, T_list=None):
    """The windowed DP + the windowed posteriors in one ragged launch each -> dict of numpy arrays."""
    from lyricalignment_amd import ops
    em, labels, n_labels, n_frames, skip, lo, hi = _pack(ems, labels_list, skips, los, his, Tmax, Lmax, T_list)
    on, off, score, vstatus = ops.viterbi_windows_batch(em, labels, n_labels, n_frames, lo, hi, skip, penalty)
    res = ops.alignment_posteriors_windows(em, labels, n_labels, n_frames, on, off, lo, hi, skip, penalty, boundary_window=window, want_gamma=True)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in zip(NAMES + ("gamma",), res)}
    out.update(onset=on.cpu().numpy(), offset=off.cpu().numpy(), score=score.cpu().numpy(), vstatus=vstatus.cpu().numpy())
    return out


def _compare(r, b, ref, em, lab, skip, lo, hi, window):
    """Clip b of launch r against the yardstick `ref` = wpr.posteriors(...) -> {output: max |difference|}, invariants included."""
    T, L = em.shape[0], len(lab)
    S = 2 * L + 1
    skip = [-1] * (L + 1) if skip is None else skip
    gamma_r, entry_r, exit_r, present_r, skip_r, log_z_r = ref
    on, off = r["onset"][b, :L], r["offset"][b, :L]
    occ_r, onp_r, offp_r = spr.scores(gamma_r, entry_r, exit_r, on, off, window)
    present = r["present_prob"][b, :L].astype(np.float64)
    span_skip = r["span_skip_prob"][b, : L + 1].astype(np.float64)
    gamma = r["gamma"][b, :T, :S].astype(np.float64)
    worst = {"occupancy": np.abs(r["occupancy"][b, :L] - occ_r).max(), "onset_prob": np.abs(r["onset_prob"][b, :L] - onp_r).max(),
             "offset_prob": np.abs(r["offset_prob"][b, :L] - offp_r).max(), "present_prob": np.abs(present - present_r).max(),
             "span_skip_prob": np.abs(span_skip - skip_r).max(), "log_z": abs(r["log_z"][b] - log_z_r),
             "gamma": np.abs(gamma - gamma_r).max(),                                              # every cell
             "gamma_rowsum": np.abs(gamma.sum(1) - 1).max(),
             "gamma_range": max(0.0, -gamma.min(), gamma.max() - 1),
             "coverage": np.abs(spr.coverage(present, span_skip, skip) - 1).max(),                # the identity, on the device's output
             "path_above_total": max(0.0, r["score"][b] - r["log_z"][b])}
    for key in PROBS:
        v = r[key][b, : L + (key == "span_skip_prob")].astype(np.float64)
        worst[key + "_range"] = max(0.0, -v.min(), v.max() - 1)
    assert not r["gamma"][b, :T, :S][~wpr.inside(T, S, lo, hi)].any()                             # exactly 0 outside the windows
    assert not r["gamma"][b, T:].any() and not r["gamma"][b, :, S:].any()
    for n in range(L):                                                                            # above 0 along the DP's reported path
        if on[n] >= 0:
            assert (r["gamma"][b, on[n]:off[n], 2 * n + 1] > 0).all(), (b, n)
    assert not r["span_skip_prob"][b, [n for n in range(L + 1) if not 0 <= skip[n] < n]].any()    # exactly 0 where no span ends
    assert not (r["occupancy"][b, :L][on < 0].any() or r["onset_prob"][b, :L][on < 0].any() or r["offset_prob"][b, :L][on < 0].any())
    return worst


def _assert_no_path(r, b, what):
    from lyricalignment_amd import _lib
    assert r["status"][b] == _lib.LA_EINFEASIBLE and r["log_z"][b] == -np.inf, what
    for key in PROBS + ("gamma",):
        assert not r[key][b].any(), (what, key)


def _forms(L):
    return [1, 0] if 2 * L + 1 <= 64 else [1]


# ------------------------------------------------------------------------------------------------ 1. every output against the yardstick
@pytest.mark.parametrize("T,L", wpr.GPU_SHAPES, ids=[f"T{t}_L{l}" for t, l in wpr.GPU_SHAPES])
def test_shapes_match_reference_and_invariants(T, L):
    """Per shape three lattices -- no spans (a null skip_from), two optional lines at penalty 0 and at penalty 1 -- two clips per launch:
    clip 0 with windows around its own best path, clip 1 around the best path of a second emission draw, so its windows bind.  Every
    output and every gamma cell against the yardstick, the invariants on the device's own output, the DPP and the LDS-exchange form of
    the one-wave kernel.  The measured maxima are printed before anything is asserted."""
    from lyricalignment_amd import _lib
    total, failed = {}, []
    for skip, pen, lab, ems, los, his, refs, feasible in wpr.gpu_cases(T, L):
        for dpp in _forms(L):
            with _lib.option("viterbi_dpp", dpp):
                r = _launch(ems, [lab, lab], None if skip is None else [skip, skip], pen, los, his)
            for c in range(2):
                what = (T, L, skip is not None, pen, dpp, c)
                if not feasible:
                    assert np.isneginf(refs[c][5])
                    _assert_no_path(r, c, what)
                    continue
                assert r["status"][c] == r["vstatus"][c] == _lib.LA_OK, what
                for k, v in _compare(r, c, refs[c], ems[c], lab, skip, los[c], his[c], 2).items():
                    total[k] = max(total.get(k, 0.0), float(v))
                    if not v <= _tol(T):
                        failed.append(what + (k, float(v), _tol(T)))
    print(f"T={T} L={L}: forms {_forms(L)}, tol={_tol(T):.2e}, measured maxima: " + json.dumps({k: float(f"{v:.2e}") for k, v in total.items()}))
    assert total and not failed, failed[:8]


# ------------------------------------------------------------------------------------------------ 2. prefetch edges
@pytest.mark.parametrize("T,L", wpr.EDGE_SHAPES, ids=[f"T{t}_L{l}" for t, l in wpr.EDGE_SHAPES])
def test_prefetch_edges(T, L):
    """T around the block depths of the emission / alpha prefetch, with spans and without; the windows stay open except that two states
    are narrowed to their segment of the path."""
    from lyricalignment_amd import _lib
    total, failed = {}, []
    for skip, pen, lab, em, lo, hi, ref, feasible in wpr.edge_cases(T, L):
        for dpp in _forms(L):
            with _lib.option("viterbi_dpp", dpp):
                r = _launch([em], [lab], None if skip is None else [skip], pen, [lo], [hi])
            what = (T, L, skip is not None, dpp)
            if not feasible:
                _assert_no_path(r, 0, what)
                continue
            assert r["status"][0] == r["vstatus"][0] == _lib.LA_OK, what
            for k, v in _compare(r, 0, ref, em, lab, skip, lo, hi, 2).items():
                total[k] = max(total.get(k, 0.0), float(v))
                if not v <= _tol(T):
                    failed.append(what + (k, float(v), _tol(T)))
    print(f"edge T={T} L={L}: tol={_tol(T):.2e}, measured maxima: " + json.dumps({k: float(f"{v:.2e}") for k, v in total.items()}))
    assert not failed, failed[:8]
    assert total or (T == 1 and L == 2)


# ------------------------------------------------------------------------------------------------ 3. all-open windows = today's entry points
@pytest.mark.parametrize("dpp", [1, 0])
def test_open_windows_equal_the_span_and_plain_posteriors_bit_for_bit(dpp):
    """conftest.e2e_cases() in one launch (one wave) and two 300-frame, 100-label clips (4 waves), every window [0, T_b): every output's
    bytes are ops.alignment_posteriors_spans' (penalties 0 and 0.75); with a null or an all -1 skip_from the shared outputs and gamma are
    ops.alignment_posteriors'."""
    import test_gpu_windows as tgw
    from lyricalignment_amd import _lib, ops
    cases = list(e2e_cases())
    small = ([c[2] for c in cases], [c[3].tolist() for c in cases])
    lab = tgw._labels(5, 100)
    big = ([tgw._emissions(1, 300, lab, 0.0), tgw._emissions(2, 300, lab, 1.5)], [lab, lab])
    n_jump_mass = 0
    for ems, labs in (small, big):
        rs = np.random.RandomState(3)
        skips = []
        for l in labs:
            row = [-1] * (len(l) + 1)
            for n in range(1, len(l) + 1):
                if rs.rand() < 0.3:
                    row[n] = int(rs.randint(max(0, n - 8), n))
            skips.append(row)
        opens = [wr.open_windows(len(l), e.shape[0]) for e, l in zip(ems, labs)]
        em, labels, n_lab, n_fr, skip, lo, hi = _pack(ems, labs, skips, [o[0] for o in opens], [o[1] for o in opens])
        none = torch.full_like(skip, -1)
        with _lib.option("viterbi_dpp", dpp):
            on, off, _, vstatus = ops.viterbi_batch(em, labels, n_lab, n_fr)
            want = ops.alignment_posteriors(em, labels, n_lab, n_fr, on, off, boundary_window=2, want_gamma=True)
            for sk, pen in ((None, 0.0), (none, 0.0), (none, 0.75)):
                got = ops.alignment_posteriors_windows(em, labels, n_lab, n_fr, on, off, lo, hi, sk, pen, boundary_window=2, want_gamma=True)
                for name, w, g in zip(SHARED + ("gamma",), want, got[:5] + got[7:]):
                    assert w.cpu().numpy().tobytes() == g.cpu().numpy().tobytes(), (name, sk is None, pen)
                assert not got[6].any() and (got[4] == vstatus).all()
                present = got[5].cpu().numpy()
                for b, l in enumerate(labs):
                    assert (present[b, : len(l)] == 1.0).all() and not present[b, len(l):].any()
            for pen in (0.0, 0.75):
                s_on, s_off, _, _ = ops.viterbi_spans_batch(em, labels, n_lab, n_fr, skip, pen)
                w_on, w_off, _, _ = ops.viterbi_windows_batch(em, labels, n_lab, n_fr, lo, hi, skip, pen)
                assert torch.equal(s_on, w_on) and torch.equal(s_off, w_off)
                want_s = ops.alignment_posteriors_spans(em, labels, n_lab, n_fr, s_on, s_off, skip, pen, boundary_window=2, want_gamma=True)
                got = ops.alignment_posteriors_windows(em, labels, n_lab, n_fr, w_on, w_off, lo, hi, skip, pen, boundary_window=2, want_gamma=True)
                for name, w, g in zip(NAMES + ("gamma",), want_s, got):
                    assert w.cpu().numpy().tobytes() == g.cpu().numpy().tobytes(), (name, pen)
                n_jump_mass += int((got[6] > 1e-3).sum())
            torch.cuda.synchronize()
        assert (vstatus == 0).all()
    assert n_jump_mass > 0


# ------------------------------------------------------------------------------------------------ 4. window edges, one ragged launch
def test_window_edges_at_the_first_and_last_frame_and_an_empty_window():
    """State 0 closed at frame 0: gamma[0, 1] is 1.  State S-1 closed at frame T-1: the path ends in S-2.  One label's state with
    lo == hi, and every state closed at frame 0: no path (LA_EINFEASIBLE, log_z -inf, every output and gamma 0)."""
    import test_gpu_windows as tgw
    from lyricalignment_amd import _lib
    T, L = 30, 4
    S = 2 * L + 1
    lab = [3, 1, 2, 3]
    em = tgw._emissions(9, T, lab, 0.0)
    o_lo, o_hi = wr.open_windows(L, T)
    los, his = [], []
    for s, a, b in ((0, 1, T), (S - 1, 0, T - 1), (5, 7, 7)):
        lo, hi = list(o_lo), list(o_hi)
        lo[s], hi[s] = a, b
        los.append(lo); his.append(hi)
    los.append([1] * S); his.append(list(o_hi))
    for skip in (None, [-1, -1, 1, -1, -1]):
        for dpp in (1, 0):
            with _lib.option("viterbi_dpp", dpp):
                r = _launch([em] * 4, [lab] * 4, None if skip is None else [skip] * 4, 0.5, los, his)
            assert r["status"].tolist() == [0, 0, 2, 2]
            for b in (0, 1):
                worst = _compare(r, b, wpr.posteriors(em, lab, los[b], his[b], skip, 0.5), em, lab, skip, los[b], his[b], 2)
                print(f"edge clip {b} spans={skip is not None} dpp={dpp}: " + json.dumps({k: float(f"{v:.2e}") for k, v in worst.items()}))
                assert all(v <= _tol(T) for v in worst.values()), worst
            g = r["gamma"]
            assert g[0, 0, 0] == 0.0 and abs(float(g[0, 0, 1]) - 1) <= _tol(T)
            assert g[1, T - 1, S - 1] == 0.0 and abs(float(g[1, T - 1, S - 2]) - 1) <= _tol(T)
            _assert_no_path(r, 2, "a label with lo == hi")
            _assert_no_path(r, 3, "every state closed at frame 0")


def test_ragged_launch_with_infeasible_empty_and_out_of_range_clips():
    """A feasible clip, a clip whose windows close every state at frame 0 (LA_EINFEASIBLE), an L = 0 clip (LA_EEMPTY), a clip whose frame
    count exceeds the launch's max_frames (LA_EINVAL) and a second feasible clip of another length in one launch, with and without spans:
    failed rows zero, the feasible clips within tolerance of the yardstick, the first one's bytes equal to its result alone."""
    import test_gpu_windows as tgw
    from lyricalignment_amd import _lib
    lab_a, lab_b = tgw._labels(1, 9), tgw._labels(2, 17)
    em_a, em_b = tgw._emissions(11, 50, lab_a, 1.5), tgw._emissions(12, 23, lab_b, 0.0)
    rs = np.random.RandomState(4)
    for spans in (False, True):
        sk_a, sk_b = (tgw._two_optional_lines(9), tgw._two_optional_lines(17)) if spans else (None, None)
        path_a = wr.viterbi_windows(tgw._emissions(13, 50, lab_a, 0.0), lab_a, *wr.open_windows(9, 50), sk_a, 0.5)[4]
        path_b = wr.viterbi_windows(tgw._emissions(14, 23, lab_b, 0.0), lab_b, *wr.open_windows(17, 23), sk_b, 0.5)[4]
        lo_a, hi_a = tgw._windows_around(rs, path_a, 19, 50)
        lo_b, hi_b = tgw._windows_around(rs, path_b, 35, 23)
        ems = [em_a, em_a, np.zeros((12, 1), np.float32), em_a, em_b]
        labs = [lab_a, lab_a, [], lab_a, lab_b]
        los = [lo_a, [1] * 19, [0], lo_a, lo_b]
        his = [hi_a, hi_a, [12], hi_a, hi_b]
        skips = [sk_a, sk_a, [-1], sk_a, sk_b] if spans else None
        r = _launch(ems, labs, skips, 0.5, los, his, T_list=[50, 50, 12, 51, 23])
        assert r["status"].tolist() == [_lib.LA_OK, _lib.LA_EINFEASIBLE, _lib.LA_EEMPTY, _lib.LA_EINVAL, _lib.LA_OK]
        assert r["status"].tolist() == r["vstatus"].tolist()
        assert r["log_z"][1] == -np.inf and r["log_z"][2] == 0.0 and r["log_z"][3] == 0.0
        for b in (1, 2, 3):
            for key in PROBS + ("gamma",):
                assert not r[key][b].any(), (b, key)
        for b, (em, lab, sk, lo, hi) in ((0, (em_a, lab_a, sk_a, lo_a, hi_a)), (4, (em_b, lab_b, sk_b, lo_b, hi_b))):
            L = len(lab)
            for key in ("occupancy", "onset_prob", "offset_prob", "present_prob"):
                assert not r[key][b, L:].any(), (b, key)
            assert not r["span_skip_prob"][b, L + 1:].any()
            worst = _compare(r, b, wpr.posteriors(em, lab, lo, hi, sk, 0.5), em, lab, sk, lo, hi, 2)
            print(f"ragged spans={spans} b={b}: tol={_tol(em.shape[0]):.2e} " + json.dumps({k: float(f"{v:.2e}") for k, v in worst.items()}))
            assert all(v <= _tol(em.shape[0]) for v in worst.values()), (b, worst)
        alone = _launch([em_a], [lab_a], [sk_a] if spans else None, 0.5, [lo_a], [hi_a], Tmax=50, Lmax=17)
        for key in NAMES + ("gamma",):
            assert alone[key][0].tobytes() == r[key][0].tobytes(), key


def test_ops_wrapper_rejects_bad_arguments():
    from lyricalignment_amd import ops
    em = torch.zeros((2, 10, 5), dtype=torch.float32).cuda()
    lab = torch.ones((2, 4), dtype=torch.int32).cuda()
    n = torch.tensor([4, 4], dtype=torch.int32).cuda()
    t = torch.tensor([10, 10], dtype=torch.int32).cuda()
    lo = torch.zeros((2, 9), dtype=torch.int32).cuda()
    hi = torch.full((2, 9), 10, dtype=torch.int32).cuda()
    skip = torch.full((2, 5), -1, dtype=torch.int32).cuda()
    on = torch.zeros((2, 4), dtype=torch.int32).cuda()
    assert ops.alignment_posteriors_windows(em, lab, n, t, on, on, lo, hi, skip)[4].tolist() == [0, 0]
    for bad in ((lo[:, :8], hi), (lo, hi[:, :8].contiguous()), (lo.long(), hi), (lo.cpu(), hi), (lo[:1], hi)):      # the DP wrapper's list
        with pytest.raises(ValueError):
            ops.alignment_posteriors_windows(em, lab, n, t, on, on, *bad)
    with pytest.raises(ValueError):
        ops.alignment_posteriors_windows(em, lab, n, t, on, on, lo, hi, skip[:, :4])
    with pytest.raises(ValueError):
        ops.alignment_posteriors_windows(em, lab, n, t, on, on, lo, hi, skip, -1.0)
    with pytest.raises(ValueError):
        ops.alignment_posteriors_windows(em, lab, n, t, on, on, lo, hi, None, float("nan"))
    with pytest.raises(ValueError):
        ops.alignment_posteriors_windows(em, lab, n, t, on, on, lo, hi, skip.long())
    with pytest.raises(ValueError):
        ops.alignment_posteriors_windows(em, lab, n, t, on, on, lo, hi, boundary_window=-1)
    with pytest.raises(ValueError):
        ops.alignment_posteriors_windows(em, lab, n, t, on[:, :3], on, lo, hi)
    with pytest.raises(NotImplementedError):
        i = torch.zeros((1, 512), dtype=torch.int32).cuda()
        ops.alignment_posteriors_windows(torch.zeros((1, 4, 513), dtype=torch.float32).cuda(), i, n[:1], t[:1], i, i,
                                         torch.zeros((1, 1025), dtype=torch.int32).cuda(), torch.zeros((1, 1025), dtype=torch.int32).cuda())


# ------------------------------------------------------------------------------------------------ 5. the Python surface on the tiny model
IDX = [0, 1, 3, 5]                                           # clips of tests/test_gpu_ragged.py: 11, 5, 8, 3 labels
SPANS = [[(0, 3), (3, 7)], [(3, 5)], [(2, 5)], []]
SCORE_KEYS = ("occupancy", "onset_prob", "offset_prob", "sung_prob", "span_skip_prob")
ALL_KEYS = set(SCORE_KEYS) | {"path_log_posterior", "window_log_prob"}


@pytest.fixture(scope="module")
def tiny():
    import test_gpu_ragged as tr
    from test_gpu_parity_full import _build
    model, _ = _build("tiny", torch.float32)
    return dict(model=model, audios=[tr._clip(i) for i in IDX], labels=tr._padded_labels(IDX), tr=tr)


def _scores_close(got, want, T, what, tol=None):
    """The probabilities and path_log_posterior within 8 T 2^-23, window_log_prob (a difference of two log_z) within 16 T 2^-23."""
    assert set(got) == set(want) == ALL_KEYS, what
    worst = 0.0
    for key in SCORE_KEYS:
        assert len(got[key]) == len(want[key]), (what, key)
        assert all(isinstance(v, float) for v in got[key])
        if len(want[key]):
            worst = max(worst, float(np.abs(np.asarray(got[key]) - np.asarray(want[key])).max()))
    worst = max(worst, abs(got["path_log_posterior"] - want["path_log_posterior"]))
    d_w = abs(got["window_log_prob"] - want["window_log_prob"])
    print(f"{what}: max |difference| {worst:.2e} (tol {tol or _tol(T):.2e}), window_log_prob {got['window_log_prob']:.4f} "
          f"|difference| {d_w:.2e} (tol {tol or 2 * _tol(T):.2e})")
    assert worst <= (tol or _tol(T)) and d_w <= (tol or 2 * _tol(T)), (what, worst, d_w)


def _coverage(score, spans):
    cov = np.asarray(score["sung_prob"], dtype=np.float64)
    for (a, n), v in zip(spans, score["span_skip_prob"]):
        cov[a:n] += v
    return cov


@pytest.mark.parametrize("use_ctc", [True, False])
def test_anchored_confidence_through_align_equals_the_two_step_route(tiny, use_ctc):
    import test_gpu_windows as tgw
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels, tr = tiny["model"], tiny["audios"], tiny["labels"], tiny["tr"]
    two = ua.perform_viterbi_ctc_anchored_scored if use_ctc else ua.perform_viterbi_anchored_scored
    n_labels = [tr.LS[i] for i in IDX]
    with torch.no_grad():
        logits, _ = model.frame_manual_forward(audios)
        T = logits.shape[1]
        free = model.align(audios, labels, use_ctc=use_ctc, return_frames=True)
        anchors, ranges = tgw._anchors_off_the_free_result(free[0].tolist(), n_labels, [T] * 4)      # the anchored onset has to move
        for spans in (None, SPANS):
            kw = dict(use_ctc=use_ctc, onset_anchors=anchors, optional_spans=spans, skip_penalty=2.0)
            what = f"use_ctc={use_ctc} spans={spans is not None}"
            seconds, scores = model.align(audios, labels, return_anchored_confidence=True, **kw)
            assert seconds == model.align(audios, labels, **kw), what
            sec2, sc2 = two(logits, labels, onset_anchors=anchors, optional_spans=spans, skip_penalty=2.0)
            assert sec2 == seconds, what
            frames = model.align(audios, labels, return_anchored_confidence=True, return_frames=True, **kw)
            assert len(frames) == 11 and all(torch.is_tensor(t) and t.is_cuda for t in frames) and frames[3].tolist() == [0] * 4
            plain_frames = model.align(audios, labels, return_frames=True, **kw)
            assert all(torch.equal(a, b) for a, b in zip(frames[:4], plain_frames))
            assert frames[7].shape == frames[10].shape == (4,) and frames[9].shape == (4, frames[8].shape[1] + 1)
            for b in range(4):
                _scores_close(scores[b], sc2[b], T, f"{what} clip {b} against the two-step route")
                assert scores[b]["window_log_prob"] == float(frames[7][b] - frames[10][b])
                assert scores[b]["window_log_prob"] <= 2 * _tol(T) and scores[b]["path_log_posterior"] <= _tol(T)
                assert all(0.0 <= v <= 1 + _tol(T) for key in SCORE_KEYS for v in scores[b][key])
                sp = (spans or [[]] * 4)[b]
                assert len(scores[b]["span_skip_prob"]) == len(sp)
                assert np.abs(_coverage(scores[b], sp) - 1).max() <= _tol(T)                         # sung_prob + the covering spans' mass
                if spans is None:
                    assert np.abs(np.asarray(scores[b]["sung_prob"]) - 1).max() == 0.0
            # the anchor moves character 1 off the frame the free alignment gave it: the unanchored model does not agree with it
            moved = [b for b, (n, _, _) in enumerate(ranges) if seconds[b][n] is not None and seconds[b][n][0] != float(int(free[0][b, n])) * HOP]
            assert len(moved) >= 2
            for b in moved:
                assert scores[b]["window_log_prob"] < 0.0, (what, b, scores[b]["window_log_prob"])
            print(f"{what}: window_log_prob {[round(s['window_log_prob'], 3) for s in scores]}, moved clips {moved}")
        # None / all-empty keywords: return_span_confidence's dicts plus window_log_prob exactly 0.0
        for spans in (None, SPANS):
            sec_s, sc_s = model.align(audios, labels, use_ctc=use_ctc, optional_spans=spans, skip_penalty=2.0, return_span_confidence=True)
            sec_a, sc_a = model.align(audios, labels, use_ctc=use_ctc, optional_spans=spans, skip_penalty=2.0, return_anchored_confidence=True,
                                      onset_anchors=[[], [], [], []], char_windows=None)
            assert sec_a == sec_s
            for b in range(4):
                assert sc_a[b]["window_log_prob"] == 0.0 and set(sc_a[b]) == ALL_KEYS
                assert {k: v for k, v in sc_a[b].items() if k != "window_log_prob"} == sc_s[b]
            assert two(logits, labels, optional_spans=spans, skip_penalty=2.0, char_windows=[[], [], [], []])[1][0]["window_log_prob"] == 0.0


def test_per_clip_long_form_lrc_and_the_refusals(tiny):
    import test_gpu_windows as tgw
    from lyricalignment_amd.harness import PinyinClassLUT, align_record_lrc
    from lyricalignment_amd.utils import alignment as ua
    from test_gpu_parity_full import VOCAB
    model, audios, labels, tr = tiny["model"], tiny["audios"], tiny["labels"], tiny["tr"]
    n_labels = [tr.LS[i] for i in IDX]
    T = [tr.TS[i] for i in IDX]
    with torch.no_grad():
        free = model.align(audios, labels, per_clip=True, return_frames=True)
        anchors, _ = tgw._anchors_off_the_free_result(free[0].tolist(), n_labels, T)
        seconds, scores = model.align(audios, labels, per_clip=True, onset_anchors=anchors, optional_spans=SPANS, skip_penalty=0.5,
                                      return_anchored_confidence=True)
        assert seconds == model.align(audios, labels, per_clip=True, onset_anchors=anchors, optional_spans=SPANS, skip_penalty=0.5)
        for r, i in enumerate(IDX):
            alone = model.align([audios[r]], tr._clip_labels(i), per_clip=True, onset_anchors=[anchors[r]], optional_spans=[SPANS[r]],
                                skip_penalty=0.5, return_anchored_confidence=True)
            assert seconds[r] == alone[0][0], i
            # a batch of one runs other GEMM tiles: its emissions differ in their last bits, the scores by far less than the 0.1 to 1 of a
            # clip that got another clip's rows, frame count, span list or windows (the bound of tests/test_gpu_span_posteriors.py)
            _scores_close(scores[r], alone[1][0], T[r], f"per_clip clip {i} in the batch against alone", tol=1e-2)
            assert np.abs(_coverage(scores[r], SPANS[r]) - 1).max() <= _tol(T[r])
        # long form: a 33 s recording (two encoder chunks, 1650 frames), an anchor in the second chunk, two optional lines
        audio = np.concatenate([tr._clip(4), tr._clip(3)])
        lab14 = torch.from_numpy(np.random.RandomState(5).randint(2, 403, size=(1, 14)))
        logits, _ = model.frame_manual_forward([audio])
        Tl = logits.shape[1]
        assert Tl > 1500
        far = [[(9, 31.0, 0.5)]]
        for spans in (None, [[(3, 7), (10, 14)]]):
            sec_l, sc_l = model.align([audio], lab14, onset_anchors=far, optional_spans=spans, return_anchored_confidence=True)
            sec_2, sc_2 = ua.perform_viterbi_ctc_anchored_scored(logits, lab14, onset_anchors=far, optional_spans=spans)
            assert sec_l == sec_2 == model.align([audio], lab14, onset_anchors=far, optional_spans=spans)
            _scores_close(sc_l[0], sc_2[0], Tl, f"long form spans={spans is not None} against the two-step route")
            assert sc_l[0]["window_log_prob"] <= 2 * _tol(Tl)
            assert np.abs(_coverage(sc_l[0], (spans or [[]])[0]) - 1).max() <= _tol(Tl)
        # the refusals
        for kw in (dict(return_confidence=True), dict(return_span_confidence=True), dict(return_confidence=True, return_span_confidence=True)):
            with pytest.raises(ValueError):
                model.align(audios, labels, onset_anchors=anchors, return_anchored_confidence=True, **kw)
            with pytest.raises(ValueError):
                model.align(audios, labels, return_anchored_confidence=True, **kw)
        with pytest.raises(ValueError):
            model.align(audios, labels, onset_anchors=anchors, return_anchored_confidence=True, skip_penalty=-1.0)
        with pytest.raises(ValueError, match="is not in list"):                      # no path inside the windows: as without the keyword
            model.align(audios, labels, per_clip=True, char_windows=[[(0, 100.0, None)], [], [], []], return_anchored_confidence=True)
    # harness.align_record_lrc(with_confidence=True): the default call's lines, sung 1 for the mandatory line
    lut = PinyinClassLUT([str(i) for i in range(VOCAB)], {str(i): i for i in range(VOCAB)})           # token id -> the same class id
    ids_all = [int(v) for v in tr._clip_labels(0)[0]]                                                 # 11 labels: lines of 3 / 4 / 2 / 2
    lines = ["".join(chr(0x4E00 + 11 * k + j) for j in range(n)) for k, n in enumerate((3, 4, 2, 2))]
    ids, pos = {}, 0
    for line in lines:
        ids[line] = ids_all[pos: pos + len(line)]
        pos += len(line)
    optional = [True, True, False, True]
    audio = tr._clip(0)
    wide = [(0.5, lines[0]), (1.0, lines[1]), (2.0, lines[2]), (3.0, lines[3])]
    # tags 0.3 s after the mandatory alignment's line starts, as tests/test_gpu_windows.py lays them: with tolerance 0.1 s they bind
    from lyricalignment_amd.harness import align_record_lines
    forced = align_record_lines(model, audio, lines, [False] * 4, lut, lambda t: ids[t])
    starts = [min(entry[0][0] + 0.3, 3.2 + 0.1 * i) for i, entry in enumerate(forced)]
    text = "[ti:test]\n" + "\n".join(f"[00:{s:05.2f}]{line}" for s, line in zip(starts, lines)) + "\n"
    tol = _tol(tr.TS[0])
    for pen, sheet, tol_s in ((0.0, wide, 10.0), (3.0, wide, 10.0), (0.0, text, 0.1), (3.0, text, 0.1)):
        want = align_record_lrc(model, audio, sheet, lut, lambda t: ids[t], tolerance_s=tol_s, optional=optional, skip_penalty=pen)
        got, conf = align_record_lrc(model, audio, sheet, lut, lambda t: ids[t], tolerance_s=tol_s, optional=optional, skip_penalty=pen,
                                     with_confidence=True)
        assert got == want and set(conf) == {"sung", "line_onset_prob", "window_log_prob"}
        assert len(conf["sung"]) == len(conf["line_onset_prob"]) == 4 and isinstance(conf["window_log_prob"], float)
        assert abs(conf["sung"][2] - 1) <= tol and got[2] is not None                                 # the mandatory line
        assert all(0.0 <= v <= 1 + tol for v in conf["sung"]) and conf["window_log_prob"] <= 2 * tol
        for entry, p in zip(got, conf["line_onset_prob"]):
            assert (p is None) == (entry is None) and (p is None or 0.0 <= p <= 1 + tol)
        if tol_s == 10.0:                                                                             # every window open: the span lattice's bits
            assert conf["window_log_prob"] == 0.0
        else:                                                                                         # tags 0.3 s off: the model disagrees
            assert conf["window_log_prob"] < 0.0
        print(f"lrc penalty {pen} tolerance {tol_s}: left out {[i for i, e in enumerate(got) if e is None]}, conf {conf}")
    mandatory = align_record_lrc(model, audio, wide, lut, lambda t: ids[t], tolerance_s=10.0, with_confidence=True)[1]
    assert all(abs(v - 1) <= tol for v in mandatory["sung"])
