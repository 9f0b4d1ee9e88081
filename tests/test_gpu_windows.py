"""Anchored alignment on the device (la_viterbi_windows_batch, ops.viterbi_windows_batch and the layers over it): bit for bit against
the float64 restatement tests/windows_reference.py (pinned on the CPU by tests/test_host_windows.py), against la_viterbi_batch /
la_viterbi_spans_batch with all-open windows, the window edges, one ragged launch, then the Python surface on the tiny random-weight
model of tests/test_gpu_ragged.py."""
import numpy as np
import pytest
import torch

import windows_reference as wr
from conftest import e2e_cases

pytestmark = pytest.mark.gpu

HOP = 0.02


def _launch(ems, labels_list, skips, penalty, los, his, T_list=None, Tmax=None):
    """Clips of different T / L in ONE la_viterbi_windows_batch launch -> host arrays (onset, offset, score, status).  skips None: a null
    skip_from.  Window rows are padded with the closed window [0, 0)."""
    from lyricalignment_amd import ops
    B = len(ems)
    Lmax = max(max(len(l) for l in labels_list), 1)
    Tmax = max(e.shape[0] for e in ems) if Tmax is None else Tmax
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
    on, off, score, status = ops.viterbi_windows_batch(em.cuda(), labels.cuda(), n_labels.cuda(), n_frames.cuda(), lo.cuda(), hi.cuda(),
                                                       None if skips is None else skip.cuda(), penalty)
    torch.cuda.synchronize()
    return on.cpu().numpy(), off.cpu().numpy(), score.cpu().numpy(), status.cpu().numpy()


def _assert_equals_reference(got, b, ref, L, what):
    """Clip b of a launch against a result of windows_reference.viterbi_windows: onset, offset, status equal, the score's bits equal."""
    on, off, score, status = got
    r_on, r_off, r_score, r_status, _ = ref
    assert status[b] == r_status, what
    assert on[b, :L].tolist() == r_on and off[b, :L].tolist() == r_off, what
    assert (on[b, L:] == -1).all() and (off[b, L:] == -1).all(), what
    assert np.float64(score[b]).tobytes() == np.float64(r_score).tobytes(), (what, float(score[b]), r_score)


def _emissions(seed, T, lab, lean):
    """Random emissions in -4 .. 0 (equal classes share a column); lean: the label columns that much lower, so that leaving labels out pays."""
    rs = np.random.RandomState(seed)
    n_classes = max(lab)
    lp = (-rs.rand(T, n_classes) * 4 - lean).astype(np.float32)
    ls = (-rs.rand(T, 1) * 4).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([ls, lp[:, np.asarray(lab) - 1]], axis=1))


def _labels(seed, L):
    rs = np.random.RandomState(seed)
    lab = [int(v) for v in rs.randint(1, (3 if L <= 4 else 50) + 1, size=L)]
    if L >= 4:
        lab[L // 2] = lab[L // 2 - 1]                      # one pair of equal neighbours
    return lab


def _two_optional_lines(L):
    """skip_from with two optional lines: four lines of about L / 4 labels, the second and the last optional (L = 2: both labels)."""
    skip = [-1] * (L + 1)
    if L < 4:
        for n in range(1, L + 1):
            skip[n] = n - 1
        return skip
    q = L // 4
    skip[2 * q] = q
    skip[L] = 3 * q
    return skip


def _windows_around(rs, path, S, T):
    """Every state's window covers its segment of `path`, widened by 0..3 frames on each side (lo may go below 0, hi beyond T: any int32
    pair is legal).  A state the path does not visit gets a window of 0..6 frames at the frame where the next visited state begins."""
    first, last = {}, {}
    for t, s in enumerate(path):
        first.setdefault(s, t)
        last[s] = t
    lo, hi = [0] * S, [0] * S
    nxt = T
    for s in range(S - 1, -1, -1):
        if s in first:
            lo[s], hi[s] = first[s] - int(rs.randint(0, 4)), last[s] + 1 + int(rs.randint(0, 4))
            nxt = first[s]
        else:
            lo[s], hi[s] = nxt - int(rs.randint(0, 4)), nxt + int(rs.randint(0, 4))
    return lo, hi


# ------------------------------------------------------------------------------------------------ 1. exact equality with the reference
SHAPES = [(40, 5), (90, 31),              # S <= 64: one wave (DPP form and LDS-exchange form)
          (100, 32),                      # 65 states: the first two-wave size
          (300, 100),                     # 4 waves
          (450, 200),                     # 8 waves
          (400, 300),                     # 16 waves, masks in LDS
          (1200, 511),                    # 16 waves, the label limit, masks in the workspace
          (7000, 20),                     # one wave, masks in the workspace
          (1, 2), (2, 2), (8, 2), (9, 2), (10, 2), (17, 2)]     # the prefetch edges: T around the depth of 8 frames


@pytest.mark.parametrize("T,L", SHAPES, ids=[f"T{t}_L{l}" for t, l in SHAPES])
def test_equals_the_float64_reference_exactly(T, L):
    """Per shape three lattices -- no spans (a null skip_from), two optional lines at penalty 0 and at penalty 1 -- each with two clips in
    one launch.  Windows are laid around a known path of the same lattice, widened by 0..3 frames per side, so the case is feasible by
    construction: clip 0 around the unconstrained restatement's path for its own emissions (the windows leave the best path in), clip 1
    around the unconstrained path of a SECOND emission draw (a valid path of the lattice that is not the best one: the windows bind, which
    the test checks against the unwindowed kernels).  Every case must be LA_OK in the restatement; none is dropped.  The one exception is
    T = 1 at L = 2, where the lattice has no path at all under any windows (start states 0 / 1, end states 3 / 4): it stays in as a case
    where kernel and restatement must agree on LA_EINFEASIBLE and on the score's bits."""
    from lyricalignment_amd import _lib, ops
    lab = _labels(7 * T + L, L)
    S = 2 * L + 1
    forms = [1, 0] if S <= 64 else [1]
    feasible = not (T == 1 and L >= 2)
    bound = 0
    for v, (skip, pen) in enumerate([(None, 0.0), (_two_optional_lines(L), 0.0), (_two_optional_lines(L), 1.0)]):
        rs = np.random.RandomState(1000 * v + 31 * T + L)
        ems = [_emissions(100 + v, T, lab, 0.0), _emissions(200 + v, T, lab, 1.5)]
        other = _emissions(300 + v, T, lab, 1.5 * (v % 2))
        refs, los, his = [], [], []
        for c, em in enumerate(ems):
            base = wr.viterbi_windows(em if c == 0 else other, lab, *wr.open_windows(L, T), skip, pen, rows=True)
            assert base[3] == (wr.LA_OK if feasible else wr.LA_EINFEASIBLE)
            lo, hi = _windows_around(rs, base[4], S, T)
            ref = wr.viterbi_windows(em, lab, lo, hi, skip, pen, rows=True)
            assert ref[3] == (wr.LA_OK if feasible else wr.LA_EINFEASIBLE), (T, L, v, c)
            refs.append(ref); los.append(lo); his.append(hi)
        for dpp in forms:
            with _lib.option("viterbi_dpp", dpp):
                got = _launch(ems, [lab, lab], None if skip is None else [skip, skip], pen, los, his)
            for c in range(2):
                _assert_equals_reference(got, c, refs[c], L, (T, L, v, c, dpp))
        # the windows of clip 1 bind: the unwindowed DP of the same lattice gives other frames or another score
        em_dev = torch.from_numpy(np.ascontiguousarray(np.stack(ems))).cuda()
        lab_dev = torch.tensor([lab, lab], dtype=torch.int32).cuda()
        nl, nf = torch.full((2,), L, dtype=torch.int32).cuda(), torch.full((2,), T, dtype=torch.int32).cuda()
        free = (ops.viterbi_batch(em_dev, lab_dev, nl, nf) if skip is None else
                ops.viterbi_spans_batch(em_dev, lab_dev, nl, nf, torch.tensor([skip, skip], dtype=torch.int32).cuda(), pen))
        assert free[0][0].tolist() == refs[0][0] and float(free[2][0]) == refs[0][2]          # clip 0: the windows leave the best path in
        bound += free[0][1].tolist() != refs[1][0] or float(free[2][1]) != refs[1][2]
    print(f"T={T} L={L}: the windows of clip 1 change the result in {bound} of 3 lattices")
    if T >= 40:                      # (the few-frame clips of the prefetch edges may leave no second path inside the widened windows)
        assert bound == 3


# ------------------------------------------------------------------------------------------------ 2. all-open windows = today's entry points
@pytest.mark.parametrize("dpp", [1, 0])
def test_open_windows_equal_viterbi_batch_and_viterbi_spans_batch_bit_for_bit(dpp):
    """conftest.e2e_cases() in one launch (one wave) and two 300-frame, 100-label clips (4 waves), every window [0, T_b): the outputs of
    ops.viterbi_batch with a null skip_from and with every entry -1, and of ops.viterbi_spans_batch with spans (penalties 0 and 0.75)."""
    from lyricalignment_amd import _lib, ops
    cases = list(e2e_cases())
    small = ([c[2] for c in cases], [c[3].tolist() for c in cases])
    lab = _labels(5, 100)
    big = ([_emissions(1, 300, lab, 0.0), _emissions(2, 300, lab, 1.5)], [lab, lab])
    n_skipped = 0
    for ems, labs in (small, big):
        B, Lmax, Tmax = len(ems), max(len(l) for l in labs), max(e.shape[0] for e in ems)
        em = torch.zeros((B, Tmax, Lmax + 1), dtype=torch.float32)
        labels = torch.zeros((B, Lmax), dtype=torch.int32)
        skip = torch.full((B, Lmax + 1), -1, dtype=torch.int32)
        rs = np.random.RandomState(3)
        for b, (e, l) in enumerate(zip(ems, labs)):
            em[b, : e.shape[0], : e.shape[1]] = torch.from_numpy(np.ascontiguousarray(e))
            labels[b, : len(l)] = torch.tensor(l, dtype=torch.int32)
            for n in range(1, len(l) + 1):
                if rs.rand() < 0.3:
                    skip[b, n] = int(rs.randint(max(0, n - 8), n))
        n_fr_host = [e.shape[0] for e in ems]
        n_lab = torch.tensor([len(l) for l in labs], dtype=torch.int32).cuda()
        n_fr = torch.tensor(n_fr_host, dtype=torch.int32).cuda()
        em, labels, skip = em.cuda(), labels.cuda(), skip.cuda()
        none = torch.full_like(skip, -1)
        lo = torch.zeros((B, 2 * Lmax + 1), dtype=torch.int32).cuda()
        hi = torch.tensor(n_fr_host, dtype=torch.int32).cuda()[:, None].repeat(1, 2 * Lmax + 1).contiguous()
        with _lib.option("viterbi_dpp", dpp):
            plain = ops.viterbi_batch(em, labels, n_lab, n_fr)
            for got in (ops.viterbi_windows_batch(em, labels, n_lab, n_fr, lo, hi), ops.viterbi_windows_batch(em, labels, n_lab, n_fr, lo, hi, none),
                        ops.viterbi_windows_batch(em, labels, n_lab, n_fr, lo, hi, none, 0.75)):
                for name, w, g in zip(("onset", "offset", "score", "status"), plain, got):
                    assert torch.equal(w, g), name
                assert plain[2].cpu().numpy().tobytes() == got[2].cpu().numpy().tobytes()
            for pen in (0.0, 0.75):
                spans = ops.viterbi_spans_batch(em, labels, n_lab, n_fr, skip, pen)
                got = ops.viterbi_windows_batch(em, labels, n_lab, n_fr, lo, hi, skip, pen)
                for name, w, g in zip(("onset", "offset", "score", "status"), spans, got):
                    assert torch.equal(w, g), (name, pen)
                assert spans[2].cpu().numpy().tobytes() == got[2].cpu().numpy().tobytes()
                n_skipped += int(((spans[0] < 0) & (torch.arange(Lmax, device=em.device)[None] < n_lab[:, None])).sum())
            torch.cuda.synchronize()
        assert (plain[3] == 0).all()
    assert n_skipped > 0


# ------------------------------------------------------------------------------------------------ 3. window edges
def test_window_edges_at_the_first_and_last_frame_and_an_empty_window():
    """State 0 and state 1 closed at frame 0 in turn: the path starts in the other one.  State S-1 closed at frame T-1: the path ends in
    S-2.  One label's state with lo == hi: no path visits every label (LA_EINFEASIBLE; the -1e7 initial value of the later states at frame 0 still
    carries a finite score, as for a clip too short for its labels).  Every state closed at frame 0: no path at all, score -inf."""
    T, L = 30, 4
    S = 2 * L + 1
    lab = [3, 1, 2, 3]
    em = _emissions(9, T, lab, 0.0)
    o_lo, o_hi = wr.open_windows(L, T)
    edits = [("state 0 closed at frame 0", 0, 1, T), ("state 1 closed at frame 0", 1, 1, T), ("state S-1 closed at frame T-1", S - 1, 0, T - 1),
             ("label 2 never allowed", 5, 7, 7)]
    los, his = [], []
    for _, s, a, b in edits:
        lo, hi = list(o_lo), list(o_hi)
        lo[s], hi[s] = a, b
        los.append(lo); his.append(hi)
    los.append([1] * S); his.append(list(o_hi))
    for skips in (None, [[-1, -1, 1, -1, -1]] * 5):
        refs = [wr.viterbi_windows(em, lab, lo, hi, None if skips is None else skips[0], 0.5) for lo, hi in zip(los, his)]
        got = _launch([em] * 5, [lab] * 5, skips, 0.5, los, his)
        for b, ref in enumerate(refs):
            _assert_equals_reference(got, b, ref, L, (b, skips is not None))
        on, off, score, status = got
        assert status[:3].tolist() == [0, 0, 0]
        assert on[0, 0] == 0 and on[1, 0] >= 1 and off[2, L - 1] == T
        assert refs[0][4][0] == 1 and refs[1][4][0] == 0 and refs[2][4][-1] == S - 2
        assert status[3] == wr.LA_EINFEASIBLE and on[3, 2] == -1
        assert status[4] == wr.LA_EINFEASIBLE and score[4] == -np.inf and (on[4] == -1).all() and (off[4] == -1).all()


# ------------------------------------------------------------------------------------------------ 4. one ragged launch
def test_ragged_launch_with_infeasible_empty_and_out_of_range_clips():
    """A feasible clip, a clip whose windows close every state at frame 0 (LA_EINFEASIBLE, every onset / offset -1, score -inf), an L = 0
    clip (LA_EEMPTY) and a clip whose frame count exceeds the launch's max_frames (LA_EINVAL) in one launch, with and without spans: the
    feasible clip's result is its result alone, and a second feasible clip of another length is the restatement's."""
    from lyricalignment_amd import _lib
    lab_a, lab_b = _labels(1, 9), _labels(2, 17)
    em_a, em_b = _emissions(11, 50, lab_a, 1.5), _emissions(12, 23, lab_b, 0.0)
    rs = np.random.RandomState(4)
    for spans in (False, True):
        sk_a, sk_b = (_two_optional_lines(9), _two_optional_lines(17)) if spans else ([-1] * 10, [-1] * 18)
        path_a = wr.viterbi_windows(_emissions(13, 50, lab_a, 0.0), lab_a, *wr.open_windows(9, 50), sk_a, 0.5)[4]
        path_b = wr.viterbi_windows(_emissions(14, 23, lab_b, 0.0), lab_b, *wr.open_windows(17, 23), sk_b, 0.5)[4]
        lo_a, hi_a = _windows_around(rs, path_a, 19, 50)
        lo_b, hi_b = _windows_around(rs, path_b, 35, 23)
        ems = [em_a, em_a, np.zeros((12, 1), np.float32), em_a, em_b]
        labs = [lab_a, lab_a, [], lab_a, lab_b]
        los = [lo_a, [1] * 19, [0], lo_a, lo_b]
        his = [hi_a, hi_a, [12], hi_a, hi_b]
        skips = [sk_a, sk_a, [-1], sk_a, sk_b] if spans else None
        got = _launch(ems, labs, skips, 0.5, los, his, T_list=[50, 50, 12, 51, 23])
        on, off, score, status = got
        alone = _launch([em_a], [lab_a], [sk_a] if spans else None, 0.5, [lo_a], [hi_a])
        assert status[0] == _lib.LA_OK == alone[3][0]
        assert on[0, :9].tolist() == alone[0][0].tolist() and off[0, :9].tolist() == alone[1][0].tolist()
        assert np.float64(score[0]).tobytes() == np.float64(alone[2][0]).tobytes()
        _assert_equals_reference(got, 0, wr.viterbi_windows(em_a, lab_a, lo_a, hi_a, sk_a, 0.5), 9, "feasible")
        assert status[1] == _lib.LA_EINFEASIBLE and score[1] == -np.inf and (on[1] == -1).all() and (off[1] == -1).all()
        assert status[2] == _lib.LA_EEMPTY and (on[2] == -1).all() and (off[2] == -1).all()
        assert status[3] == _lib.LA_EINVAL and (on[3] == -1).all() and (off[3] == -1).all()
        ref_b = wr.viterbi_windows(em_b, lab_b, lo_b, hi_b, sk_b, 0.5)
        assert ref_b[3] == wr.LA_OK
        _assert_equals_reference(got, 4, ref_b, 17, "second feasible clip")


def test_ops_wrapper_rejects_bad_arguments():
    from lyricalignment_amd import ops
    em = torch.zeros((2, 10, 5), dtype=torch.float32).cuda()
    lab = torch.ones((2, 4), dtype=torch.int32).cuda()
    n = torch.tensor([4, 4], dtype=torch.int32).cuda()
    t = torch.tensor([10, 10], dtype=torch.int32).cuda()
    lo = torch.zeros((2, 9), dtype=torch.int32).cuda()
    hi = torch.full((2, 9), 10, dtype=torch.int32).cuda()
    skip = torch.full((2, 5), -1, dtype=torch.int32).cuda()
    assert ops.viterbi_windows_batch(em, lab, n, t, lo, hi, skip)[3].tolist() == [0, 0]
    for bad in ((lo[:, :8], hi), (lo, hi[:, :8].contiguous()), (lo.long(), hi), (lo.cpu(), hi), (lo[:1], hi)):
        with pytest.raises(ValueError):
            ops.viterbi_windows_batch(em, lab, n, t, *bad)
    with pytest.raises(ValueError):
        ops.viterbi_windows_batch(em, lab, n, t, lo, hi, skip[:, :4])
    with pytest.raises(ValueError):
        ops.viterbi_windows_batch(em, lab, n, t, lo, hi, skip, -1.0)
    with pytest.raises(ValueError):
        ops.viterbi_windows_batch(em, lab, n, t, lo, hi, None, float("nan"))
    with pytest.raises(NotImplementedError):
        ops.viterbi_windows_batch(torch.zeros((1, 4, 513), dtype=torch.float32).cuda(), torch.ones((1, 512), dtype=torch.int32).cuda(),
                                  n[:1], t[:1], torch.zeros((1, 1025), dtype=torch.int32).cuda(), torch.zeros((1, 1025), dtype=torch.int32).cuda())


# ------------------------------------------------------------------------------------------------ 5. the Python surface on the tiny model
IDX = [0, 1, 3, 5]                                           # clips of tests/test_gpu_ragged.py: 11, 5, 8, 3 labels
SPANS = [[(0, 3), (3, 7)], [(3, 5)], [(2, 5)], []]
TOL = 2 * HOP


@pytest.fixture(scope="module")
def tiny():
    import test_gpu_ragged as tr
    from test_gpu_parity_full import _build
    model, _ = _build("tiny", torch.float32)
    return dict(model=model, audios=[tr._clip(i) for i in IDX], labels=tr._padded_labels(IDX), tr=tr)


def _anchors_off_the_free_result(on, n_labels, T):
    """One onset anchor per clip, on character 1, four frames after the frame the unanchored alignment gave it (kept inside the clip so that
    a path exists), tolerance two frames -> (anchors, [(n, f_lo, f_hi)] per clip): the anchored onset has to move."""
    anchors, ranges = [], []
    for b, L in enumerate(n_labels):
        f = min(max(int(on[b][1]) + 4, 3), T[b] - L - 4)
        anchors.append([(1, f * HOP, TOL)])
        ranges.append((1, f - 2, f + 2))
    return anchors, ranges


@pytest.mark.parametrize("use_ctc", [True, False])
def test_align_with_anchors_equals_the_two_step_route(tiny, use_ctc):
    from lyricalignment_amd import _lib, ops
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels, tr = tiny["model"], tiny["audios"], tiny["labels"], tiny["tr"]
    two = ua.perform_viterbi_ctc if use_ctc else ua.perform_viterbi
    n_labels = [tr.LS[i] for i in IDX]
    with torch.no_grad():
        logits, _ = model.frame_manual_forward(audios)
        T = logits.shape[1]
        free = model.align(audios, labels, use_ctc=use_ctc, return_frames=True)
        anchors, ranges = _anchors_off_the_free_result(free[0].tolist(), n_labels, [T] * 4)
        for spans in (None, SPANS):
            fused = model.align(audios, labels, use_ctc=use_ctc, onset_anchors=anchors, optional_spans=spans, skip_penalty=2.0)
            assert fused == two(logits, labels, onset_anchors=anchors, optional_spans=spans, skip_penalty=2.0)
            on, off, score, status = model.align(audios, labels, use_ctc=use_ctc, onset_anchors=anchors, optional_spans=spans, skip_penalty=2.0,
                                                 return_frames=True)
            assert status.tolist() == [0] * 4
            # the two steps by hand: emissions, then the windowed DP
            lab_dev, n_lab, lists = ua._labels_to_device(labels, 4, logits.device)
            em = ops.emissions_from_logits(logits.float().contiguous(), lab_dev, n_lab, _lib.LA_VARIANT_CTC if use_ctc else _lib.LA_VARIANT_PLAIN)
            lo, hi = ua._windows_of(None, anchors, lists, [T] * 4, HOP)
            skip = ua._skip_from_of_spans(spans, lists)
            by_hand = ops.viterbi_windows_batch(em, lab_dev, n_lab, torch.full((4,), T, dtype=torch.int32, device=em.device), lo.cuda(), hi.cuda(),
                                                None if skip is None else skip.cuda(), 2.0)
            # frames and status equal; the scores are sums of T emissions that the fused head and emissions_from_logits round separately
            # (float32 log-softmax values below 32 in magnitude, ulp 2^-19; four ulp per frame allowed)
            assert torch.equal(on, by_hand[0]) and torch.equal(off, by_hand[1]) and torch.equal(status, by_hand[3])
            worst = float((score - by_hand[2]).abs().max())
            print(f"use_ctc={use_ctc} spans={spans is not None}: max |score - two-step score| {worst:.2e} (bound {T * 4 * 2.0 ** -19:.2e})")
            assert worst <= T * 4 * 2.0 ** -19
            moved = 0
            for b, (n, f_lo, f_hi) in enumerate(ranges):
                v = int(on[b, n])
                assert v < 0 or f_lo <= v <= f_hi, (b, v, f_lo, f_hi)
                assert v < 0 or fused[b][n][0] == float(v) * HOP
                moved += v >= 0 and v != int(free[0][b, n])
            assert moved >= 2
        # None / all-empty keywords: the call as it was; several anchors and a character window together
        plain = model.align(audios, labels, use_ctc=use_ctc)
        assert model.align(audios, labels, use_ctc=use_ctc, onset_anchors=None, char_windows=[[], [], [], []]) == plain
        assert two(logits, labels, onset_anchors=[[], [], [], []]) == two(logits, labels)
        cw = [[(0, None, (int(free[1][b, 0]) + 3) * HOP)] for b in range(4)]
        both = model.align(audios, labels, use_ctc=use_ctc, onset_anchors=anchors, char_windows=cw)
        assert both == two(logits, labels, onset_anchors=anchors, char_windows=cw)
        for b in range(4):
            assert both[b][0][1] <= (int(free[1][b, 0]) + 3) * HOP + 1e-9


def test_per_clip_and_long_form_with_anchors_and_refused_keywords(tiny):
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels, tr = tiny["model"], tiny["audios"], tiny["labels"], tiny["tr"]
    n_labels = [tr.LS[i] for i in IDX]
    T = [tr.TS[i] for i in IDX]
    with torch.no_grad():
        free = model.align(audios, labels, per_clip=True, return_frames=True)
        anchors, ranges = _anchors_off_the_free_result(free[0].tolist(), n_labels, T)
        lg = model.frame_logits_per_clip(audios)
        pad = torch.nn.utils.rnn.pad_sequence(lg, batch_first=True)
        for spans in (None, SPANS):
            batch = model.align(audios, labels, per_clip=True, onset_anchors=anchors, optional_spans=spans)
            assert batch == ua.perform_viterbi_ctc(pad, labels, n_frames=T, onset_anchors=anchors, optional_spans=spans)
            for r, i in enumerate(IDX):
                alone = model.align([audios[r]], tr._clip_labels(i), per_clip=True, onset_anchors=[anchors[r]],
                                    optional_spans=None if spans is None else [spans[r]])
                assert batch[r] == alone[0], i
                n, f_lo, f_hi = ranges[r]
                assert batch[r][n] is None or f_lo * HOP - 1e-9 <= batch[r][n][0] <= f_hi * HOP + 1e-9
        # the long form: a 33 s recording (two encoder chunks, 1650 frames), an anchor in the second chunk
        audio = np.concatenate([tr._clip(4), tr._clip(3)])
        long_labels = torch.from_numpy(np.random.RandomState(5).randint(2, 403, size=(1, 14)))
        logits, _ = model.frame_manual_forward([audio])
        assert logits.shape[1] > 1500
        far = [[(9, 31.0, 0.5)]]
        for spans in (None, [[(3, 7), (10, 14)]]):
            got = model.align([audio], long_labels, onset_anchors=far, optional_spans=spans)
            assert got == ua.perform_viterbi_ctc(logits, long_labels, onset_anchors=far, optional_spans=spans)
            assert got[0][9] is None or 30.5 - 1e-9 <= got[0][9][0] <= 31.5 + 1e-9
        assert got[0][9] is not None or spans is not None
        # no posteriors on the windowed lattice
        for kw in (dict(return_confidence=True), dict(return_span_confidence=True), dict(return_confidence=True, per_clip=True)):
            with pytest.raises(ValueError):
                model.align(audios, labels, onset_anchors=anchors, **kw)
        with pytest.raises(ValueError):
            model.align(audios, labels, char_windows=[[(0, 0.0, 1.0)], [], [], []], return_confidence=True)
        with pytest.raises(ValueError):
            ua.perform_viterbi_ctc_scored(pad, labels, n_frames=T, onset_anchors=anchors)
        with pytest.raises(ValueError):
            ua.perform_viterbi_scored(pad, labels, n_frames=T, char_windows=[[(0, 0.0, 1.0)], [], [], []])
        for bad in (dict(onset_anchors=[[(11, 0.1, 0.1)], [], [], []]), dict(onset_anchors=[[(0, 0.1, -1.0)], [], [], []]),
                    dict(onset_anchors=[[], [], []]), dict(char_windows=[[(0, float("nan"), None)], [], [], []])):
            with pytest.raises(ValueError):
                model.align(audios, labels, **bad)
        # a clip without a path inside its windows is reported like a clip too short for its labels
        with pytest.raises(ValueError, match="is not in list"):
            model.align(audios, labels, per_clip=True, char_windows=[[(0, 100.0, None)], [], [], []])


def test_align_record_lrc(tiny):
    from lyricalignment_amd.harness import PinyinClassLUT, align_record_lines, align_record_lrc
    from test_gpu_parity_full import VOCAB
    model, tr = tiny["model"], tiny["tr"]
    lut = PinyinClassLUT([str(i) for i in range(VOCAB)], {str(i): i for i in range(VOCAB)})           # token id -> the same class id
    ids_all = [int(v) for v in tr._clip_labels(0)[0]]                                                 # 11 labels: lines of 3 / 4 / 2 / 2
    lines = ["".join(chr(0x4E00 + 11 * k + j) for j in range(n)) for k, n in enumerate((3, 4, 2, 2))]
    ids, pos = {}, 0
    for line in lines:
        ids[line] = ids_all[pos: pos + len(line)]
        pos += len(line)
    optional = [True, True, False, True]
    audio = tr._clip(0)                                                                               # 3.76 s
    # a tolerance wider than the clip: every window is open, the result is align_record_lines', skipped lines included
    wide = [(0.5, lines[0]), (1.0, lines[1]), (2.0, lines[2]), (3.0, lines[3])]
    for pen in (0.0, 3.0):
        want = align_record_lines(model, audio, lines, optional, lut, lambda t: ids[t], use_ctc_loss=True, skip_penalty=pen)
        got = align_record_lrc(model, audio, wide, lut, lambda t: ids[t], tolerance_s=10.0, optional=optional, skip_penalty=pen)
        assert got == want
    assert align_record_lrc(model, audio, wide, lut, lambda t: ids[t], tolerance_s=10.0) == \
        align_record_lines(model, audio, lines, [False] * 4, lut, lambda t: ids[t])
    # LRC text with tags 0.3 s after the mandatory alignment's line starts, tolerance 0.1 s: every sung line starts within 0.1 s of its tag,
    # and None stands for exactly the lines the span DP skipped
    forced = align_record_lines(model, audio, lines, [False] * 4, lut, lambda t: ids[t])
    starts = [min(entry[0][0] + 0.3, 3.2 + 0.1 * i) for i, entry in enumerate(forced)]
    text = "[ti:test]\n" + "\n".join(f"[00:{s:05.2f}]{line}" for s, line in zip(starts, lines)) + "\n"
    for pen in (0.0, 3.0):
        got = align_record_lrc(model, audio, text, lut, lambda t: ids[t], tolerance_s=0.1, optional=optional, skip_penalty=pen)
        anchors = [[(p, round(s, 2), 0.1) for p, s in zip((0, 3, 7, 9), starts)]]
        with torch.no_grad():
            chars = model.align([audio], tr._clip_labels(0), use_ctc=True, optional_spans=[[(0, 3), (3, 7), (9, 11)]], skip_penalty=pen,
                                onset_anchors=anchors)[0]
        assert len(got) == 4 and got[2] is not None
        pos = 0
        for line, entry, s in zip(lines, got, starts):
            part = chars[pos: pos + len(line)]
            pos += len(line)
            if entry is None:
                assert all(c is None for c in part)
            else:
                assert entry == [[c[0], c[1], ch] for c, ch in zip(part, line)]
                assert abs(entry[0][0] - round(s, 2)) <= 0.1 + 0.02 + 1e-9            # (the range is widened to the frame nearest to the tag)
        print(f"penalty {pen}: lines left out {[i for i, e in enumerate(got) if e is None]}")
    with pytest.raises(ValueError):
        align_record_lrc(model, audio, "[ar:nobody]\n", lut, lambda t: ids[t])
