"""Confidence for free line order on the device (la_alignment_posteriors_lines, ops.alignment_posteriors_lines and the layers over it):
every output and every gamma cell against the all-pairs float64 forward-backward tests/line_posterior_reference.py (pinned by
tests/test_host_line_posteriors.py) in every kernel form, within the project's bound 8 T 2^-23 max(1, |value|); a soft case over a
two-class alphabet; the cancellation case that a subtractive or fixed-shift hub fails; a clip alone against the clip in a batch; two
calls; penalty +inf against la_alignment_posteriors; one line against la_alignment_posteriors_repeats; statuses; then the Python surface
on the tiny random-weight model and the bench tool.

Measured on an MI355X (maximum of |device - yardstick| / max(1, |yardstick|) over every output, in units of the bound): at most 0.0096
(gamma of the 5 x 24 case), log_z at most 0.0004; the table is in DESIGN.md "Posteriors on the line-order lattice".  Every test prints
its figures before it asserts."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import line_order_reference as lo
import line_posterior_reference as lp
from conftest import ROOT

pytestmark = pytest.mark.gpu

HOP = 0.02
PEN = 1.0
WINDOW = 2


def bound(T):
    return 8.0 * T * 2.0 ** -23


def _labels(L):
    return [1 + n % 37 for n in range(L)]


# labels x frames -> (frames, line lengths, the lines sung in order, frames per label, frames of silence after a line); the kernel form in
# the id.  The far right and the far left of the sheet are sung, so the last and the first threads of the workgroup carry the path.
SHAPES = {
    "one_wave_5x24": (24, [2, 3], [1, 1, 1], 2, 1),
    "two_waves_40x200": (200, [8] * 5, [1, 0, 2, 4, 4], 2, 1),
    "nw16_300x96": (96, [30] * 10, [9, 0], 1, 1),
    "r2_520x96": (96, [26] * 20, [19, 0], 1, 1),
    "r4_1030x96": (96, [10] * 103, [102, 0, 50], 1, 1),
    "r8_2050x96": (96, [10] * 205, [204, 0, 100], 1, 1),
    "r8_4095x64": (64, [15] * 273, [272, 0, 136], 1, 1),
}


@functools.lru_cache(maxsize=None)
def clip_and_reference(name, pen=PEN):
    """-> the planted clip, the DP restatement's result and the yardstick's posteriors (computed once, shared, never written to)"""
    T, lengths, sung, seg, gap = SHAPES[name]
    c = lo.planted(len(name), T, lengths, sung, seg, gap, labels=_labels(sum(lengths)))
    return c, lo.viterbi(c["em"], c["lab"], c["ls"], pen), lp.posteriors(c["em"], c["lab"], c["ls"], pen)


def _pad(Lmax):
    """A clip that only keeps the kernel form of a batch (T = 0: LA_EINVAL)"""
    return dict(lab=[1] * Lmax, em=np.zeros((8, Lmax + 1), np.float32), ls=[1] + [0] * (Lmax - 1), T=0)


def _run(clips, pen=PEN, window=WINDOW, want_gamma=True):
    """Clips of different T / L in ONE la_viterbi_lines_batch and ONE la_alignment_posteriors_lines launch -> dict of host arrays."""
    from lyricalignment_amd import ops
    B = len(clips)
    Lmax = max(max(len(c["lab"]) for c in clips), 1)
    Tmax = max(c["em"].shape[0] for c in clips)
    em = torch.zeros((B, Tmax, Lmax + 1), dtype=torch.float32)
    labels = torch.zeros((B, Lmax), dtype=torch.int32)
    ls = torch.zeros((B, Lmax), dtype=torch.int32)
    for b, c in enumerate(clips):
        e, l = c["em"], c["lab"]
        em[b, : e.shape[0], : e.shape[1]] = torch.from_numpy(e)
        labels[b, : len(l)] = torch.tensor(list(l), dtype=torch.int32)
        ls[b, : len(l)] = torch.tensor(c["ls"], dtype=torch.int32)
    args = (em.cuda(), labels.cuda(), torch.tensor([len(c["lab"]) for c in clips], dtype=torch.int32).cuda(),
            torch.tensor([c["T"] for c in clips], dtype=torch.int32).cuda())
    ls = ls.cuda()
    on, off, score, dp_status, path = ops.viterbi_lines_batch(*args, ls, pen)
    out = ops.alignment_posteriors_lines(*args, on, off, ls, pen, path, window, want_gamma=want_gamma)
    torch.cuda.synchronize()
    keys = ("occupancy", "onset_prob", "offset_prob", "log_z", "status", "visits", "in_order", "path_prob") + (("gamma",) if want_gamma else ())
    got = {k: t.cpu().numpy() for k, t in zip(keys, out)}
    got.update(onset=on.cpu().numpy(), offset=off.cpu().numpy(), score=score.cpu().numpy(), dp_status=dp_status.cpu().numpy(),
               path=path.cpu().numpy())
    return got


def _expected(ref, dp, window=WINDOW):
    """The yardstick's posteriors and the DP's frames -> the entry's outputs for one clip"""
    occ, onp, offp = lp.scores(ref, dp[0], dp[1], window)
    return dict(occupancy=occ, onset_prob=onp, offset_prob=offp, visits=ref["visits"], in_order=ref["in_order"],
                path_prob=lp.path_prob(ref, dp[4]), gamma=ref["gamma"], log_z=np.float64(ref["log_z"]))


def _assert_within_bound(got, b, c, want, what, keys=None):
    """Every output of clip b within the bound of `want`; cells beyond the clip's labels / frames are zero -> the largest error in units
    of the bound"""
    L, T = len(c["lab"]), c["T"]
    S = 2 * L + 1
    tol = bound(T)
    worst = {}
    assert got["status"][b] == lo.LA_OK, (what, got["status"][b])
    for k in keys or ("occupancy", "onset_prob", "offset_prob", "visits", "in_order", "path_prob", "gamma", "log_z"):
        if k not in got or k not in want:
            continue
        g = np.asarray(got[k][b], np.float64)
        w = np.asarray(want[k], np.float64)
        if k == "gamma":
            assert not g[T:].any() and not g[:, S:].any(), (what, k)
            g = g[:T, :S]
        elif k == "path_prob":
            assert not g[T:].any(), (what, k)
            g = g[:T]
        elif k != "log_z":
            assert not g[L:].any(), (what, k)
            g = g[:L]
        assert np.isfinite(g).all(), (what, k)
        err = np.abs(g - w) / np.maximum(1.0, np.abs(w))
        worst[k] = float(err.max()) / tol
    print(f"{what}: T {T}, bound {tol:.3e}, largest error / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (what, k, v)
    return worst


def _assert_not_vacuous(c, dp, ref, what):
    """On the yardstick alone: a line surely sung and a line surely not, at least 1.5 expected arrivals out of print order, and a best path
    with a free start or a free end."""
    starts = lo.line_starts_of(c["ls"], len(c["lab"]))
    line_visits = ref["visits"][starts]
    assert (line_visits > 0.99).any() and (line_visits < 0.01).any(), (what, line_visits)
    assert (ref["visits"][starts] - ref["in_order"][starts]).sum() >= 1.5, what
    assert dp.free_start or dp.free_end, what
    for a, e in zip(starts, starts[1:] + [len(c["lab"])]):                     # visits is constant along a line
        assert np.allclose(ref["visits"][a:e], ref["visits"][a], rtol=0, atol=1e-9), (what, a)
    assert np.allclose(ref["gamma"].sum(1), 1.0, rtol=0, atol=1e-9), what


# ------------------------------------------------------------------------------------------------ 1. the yardstick, every kernel form
@pytest.mark.parametrize("name", list(SHAPES))
def test_device_equals_the_all_pairs_forward_backward(name):
    c, dp, ref = clip_and_reference(name)
    _assert_not_vacuous(c, dp, ref, name)
    got = _run([c])
    assert got["path"][0, : c["T"]].tolist() == dp[4] and got["dp_status"][0] == lo.LA_OK
    if name == "r8_4095x64":                                    # the forward sweep alone gives the same log_z
        assert abs(lp.log_z_only(c["em"], c["lab"], c["ls"], PEN) - ref["log_z"]) <= 1e-9
    _assert_within_bound(got, 0, c, _expected(ref, dp), name)


@functools.lru_cache(maxsize=None)
def soft_clips():
    clips = []
    for seed, (L, T, n_lines) in enumerate(((9, 30, 4), (40, 60, 9), (300, 96, 40))):
        rs = np.random.RandomState(100 + seed)
        cuts = sorted(rs.choice(np.arange(1, L), size=n_lines - 1, replace=False).tolist())
        lengths = np.diff([0] + cuts + [L]).tolist()
        c = lo.planted(seed, T, lengths, [], vocab=2)
        c["em"] = np.ascontiguousarray(np.log(rs.dirichlet(np.ones(L + 1), size=T)).astype(np.float32))
        clips.append(c)
    return clips


@pytest.mark.parametrize("pen", [0.0, 0.3])
def test_soft_emissions_over_two_classes(pen):
    """Unplanted noise over a two-class alphabet: every line end collides with line starts, mass everywhere, lines sung more than once in
    expectation; one wave, two waves and sixteen."""
    clips = soft_clips()
    dps = [lo.viterbi(c["em"], c["lab"], c["ls"], pen) for c in clips]
    refs = [lp.posteriors(c["em"], c["lab"], c["ls"], pen) for c in clips]
    for c, r in zip(clips, refs):
        src, cls = lo.sources(c["lab"], c["ls"])
        starts = lo.line_starts_of(c["ls"], len(c["lab"]))
        ends = {k for k in cls if k is not None}
        assert all(any(c["lab"][a] == k for a in starts) for k in ends)              # every line end's class begins some line
        assert (r["visits"] > 1.2).any(), r["visits"].max()
    for b, (c, dp, r) in enumerate(zip(clips, dps, refs)):
        got = _run([c], pen)                                                          # each in its own kernel form
        _assert_within_bound(got, 0, c, _expected(r, dp), f"soft clip {b} penalty {pen}")


# ------------------------------------------------------------------------------------------------ 2. the cancellation case
@pytest.mark.parametrize("pen", [0.0, 0.7])
def test_a_target_whose_allowed_sources_lie_750_nats_below_the_excluded_one(pen):
    """Two lines; line 0 ends in class 7 and line 1 begins with class 7.  At frame 2 line 0's last label holds all the mass: every source
    that line 1's first label may be entered from lies more than 750 nats below it.  The path nevertheless enters line 1 at frame 3,
    through the silence.  A hub that subtracts the excluded class from a total, or scales every source by the frame's best, gives that
    target nothing."""
    labels, ls, T = [5, 7, 7, 9], [1, 0, 1, 0], 6
    em = np.full((T, 5), -1000.0, np.float32)
    for t, col in enumerate([1, 2, 2, 3, 4, 0]):               # labels 0, 1, 1, then 2, 3 and the closing silence
        em[t, col] = 0.0
    em[2, 0] = -800.0                                           # the silence after line 0, one frame early
    c = dict(lab=labels, em=em, ls=ls, T=T)
    lat = lp.Lattice(labels, ls)
    alpha = lp.forward(em, lat, pen)[1]
    target, excluded = 5, 3
    allowed = [int(s) for j, s in enumerate(lat.src) if s != excluded]
    assert labels[excluded >> 1] == labels[target >> 1]
    assert all(alpha[2, excluded] - alpha[2, s] > 750.0 for s in allowed), alpha[2]
    ref = lp.posteriors(em, labels, ls, pen)
    assert ref["gamma"][3, target] > 0.3, ref["gamma"][3]
    dp = lo.viterbi(em, labels, ls, pen)
    got = _run([c], pen)
    _assert_within_bound(got, 0, c, _expected(ref, dp), f"cancellation penalty {pen}")


# ------------------------------------------------------------------------------------------------ 3. alone = in a batch; two calls
def test_a_clip_in_a_ragged_batch_equals_the_clip_alone_and_two_calls_agree():
    names = ["one_wave_5x24", "nw16_300x96", "two_waves_40x200"]
    clips = [clip_and_reference(n)[0] for n in names]
    first, second = _run(clips), _run(clips)
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), k
    Lmax = max(len(c["lab"]) for c in clips)
    for b, (c, n) in enumerate(zip(clips, names)):
        _, dp, ref = clip_and_reference(n)
        _assert_within_bound(first, b, c, _expected(ref, dp), f"{n} in the batch")
        alone = _run([c, _pad(Lmax)])                                                 # (the pad keeps the kernel form)
        L, T = len(c["lab"]), c["T"]
        for k in ("occupancy", "onset_prob", "offset_prob", "visits", "in_order"):
            assert alone[k][0, :L].tobytes() == first[k][b, :L].tobytes(), (n, k)
        assert alone["log_z"][0].tobytes() == first["log_z"][b].tobytes()
        assert alone["path_prob"][0, :T].tobytes() == first["path_prob"][b, :T].tobytes()
        assert np.ascontiguousarray(alone["gamma"][0, :T, : 2 * L + 1]).tobytes() == np.ascontiguousarray(first["gamma"][b, :T, : 2 * L + 1]).tobytes()


# ------------------------------------------------------------------------------------------------ 4. the two identities
@pytest.mark.parametrize("name", ["two_waves_40x200", "r2_520x96"])
def test_an_infinite_penalty_is_the_plain_lattice(name):
    from lyricalignment_amd import ops
    T, lengths, _, _, _ = SHAPES[name]
    L = sum(lengths)
    T = max(T, L + 8)
    c = lo.planted(7, T, lengths, list(range(len(lengths))), 1, 0, labels=_labels(L))      # sung straight through
    got = _run([c], float("inf"))
    args = (torch.from_numpy(c["em"])[None].cuda(), torch.tensor([c["lab"]], dtype=torch.int32).cuda(),
            torch.tensor([L], dtype=torch.int32).cuda(), torch.tensor([T], dtype=torch.int32).cuda())
    on, off, _, st = ops.viterbi_batch(*args)
    if L <= 511:
        want = ops.alignment_posteriors(*args, on, off, WINDOW, want_gamma=True)
    else:                                                       # the same lattice beyond 511 labels: the whole-song entry, no span, no window
        want = ops.alignment_posteriors_lattice(*args, on, off, boundary_window=WINDOW, want_gamma=True)
        want = want[:5] + want[-1:]
    torch.cuda.synchronize()
    assert st.item() == lo.LA_OK and got["onset"].tobytes() == on.cpu().numpy().tobytes()
    plain = dict(zip(("occupancy", "onset_prob", "offset_prob", "log_z", "status", "gamma"), (t.cpu().numpy()[0] for t in want)))
    plain["visits"] = np.ones(L)
    plain["in_order"] = np.asarray(c["ls"], np.float64)
    _assert_within_bound(got, 0, c, plain, f"penalty inf {name}")


@pytest.mark.parametrize("L,T", [(26, 120), (300, 620)])
def test_a_single_line_is_the_repeat_lattice_with_the_whole_sheet_repeatable(L, T):
    """(One line has to be sung from its first label to its last: T cannot stay below L here.)"""
    from lyricalignment_amd import ops
    c = lo.planted(L, T, [L], [0, 0], 2 if L == 26 else 1, 2, labels=_labels(L))       # the sheet sung twice
    got = _run([c], 0.5)
    rf = torch.full((1, L), -1, dtype=torch.int32)
    rf[0, 0] = L
    args = (torch.from_numpy(c["em"])[None].cuda(), torch.tensor([c["lab"]], dtype=torch.int32).cuda(),
            torch.tensor([L], dtype=torch.int32).cuda(), torch.tensor([T], dtype=torch.int32).cuda())
    dp = ops.viterbi_repeats_batch(*args, repeat_from=rf.cuda(), repeat_penalty=0.5)
    want = ops.alignment_posteriors_repeats(*args, dp[0], dp[1], repeat_from=rf.cuda(), repeat_penalty=0.5, path=dp[4],
                                            boundary_window=WINDOW, want_gamma=True)
    torch.cuda.synchronize()
    assert got["path"].tobytes() == dp[4].cpu().numpy().tobytes() and got["onset"].tobytes() == dp[0].cpu().numpy().tobytes()
    keys = ("occupancy", "onset_prob", "offset_prob", "log_z", "status", "visits", "span_skip", "repeat_count", "path_prob", "gamma")
    rep = dict(zip(keys, (t.cpu().numpy()[0] for t in want)))
    assert rep["status"] == lo.LA_OK
    assert rep["repeat_count"][0] > 0.99                                               # the return is taken
    worst = _assert_within_bound(got, 0, c, rep, f"one line {L} x {T}",
                                 keys=("occupancy", "onset_prob", "offset_prob", "visits", "path_prob", "gamma", "log_z"))
    assert worst
    # visits - in_order at label 0 = the returns (two device numbers, each within the bound of its own yardstick)
    assert abs((got["visits"][0, 0] - got["in_order"][0, 0]) - rep["repeat_count"][0]) <= 2 * bound(T) * max(1.0, rep["visits"][0])
    assert not got["in_order"][0, 1:].any()


# ------------------------------------------------------------------------------------------------ 5. statuses
def test_a_clip_without_a_first_line_is_einval_and_its_batch_mates_are_unaffected():
    from lyricalignment_amd import ops
    good, dp, ref = clip_and_reference("two_waves_40x200")
    bad = dict(good, ls=[0] + good["ls"][1:])
    got = _run([good, bad, good])
    for b in (0, 2):
        _assert_within_bound(got, b, good, _expected(ref, dp), f"clip {b} beside the invalid one")
    assert got["status"][1] == lo.LA_EINVAL and got["log_z"][1] == 0.0
    for k in ("occupancy", "onset_prob", "offset_prob", "visits", "in_order", "path_prob", "gamma"):
        assert not got[k][1].any(), k
    alone = _run([good, _pad(len(good["lab"]))])
    for k in ("occupancy", "visits", "in_order", "log_z", "gamma"):
        assert alone[k][0].tobytes() == got[k][0].tobytes() == got[k][2].tobytes(), k
    # too few frames under a prohibitive penalty: no path
    short = dict(good, em=good["em"][:20], T=20)
    got = _run([short], float("inf"))
    assert got["status"][0] == lo.LA_EINFEASIBLE and got["log_z"][0] == -np.inf and not got["gamma"].any() and not got["visits"].any()
    em = torch.from_numpy(good["em"])[None].cuda()
    args = (em, torch.tensor([good["lab"]], dtype=torch.int32).cuda(), torch.tensor([40], dtype=torch.int32).cuda(),
            torch.tensor([200], dtype=torch.int32).cuda())
    z = torch.zeros((1, 40), dtype=torch.int32).cuda()
    for pen in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="line_jump_penalty"):
            ops.alignment_posteriors_lines(*args, z, z, torch.tensor([good["ls"]], dtype=torch.int32).cuda(), pen)


# ------------------------------------------------------------------------------------------------ 6. the Python surface
@pytest.fixture(scope="module")
def tiny():
    import test_gpu_ragged as tr
    from test_gpu_parity_full import _build
    model, _ = _build("tiny", torch.float32)
    idx = [0, 1, 3, 5]                                           # clips of tests/test_gpu_ragged.py: 11, 5, 8, 3 labels
    return dict(model=model, audios=[tr._clip(i) for i in idx], labels=tr._padded_labels(idx), tr=tr, idx=idx)


LINE_STARTS = [[0, 3, 7, 9], [0, 2], [0, 1, 4], [0]]


def _flags(starts, L):
    return [1 if n in starts else 0 for n in range(L)]


def _expected_scores(em, lists, counts, line_starts, pen):
    """The yardstick on a device emission matrix [B, T, >= L+1] (host array) -> seconds, segments, score dicts as the public functions give them"""
    seconds, segments, dicts = [], [], []
    for b, labs in enumerate(lists):
        L = len(labs)
        e, flags = em[b, : counts[b], : L + 1], _flags(line_starts[b], L)
        r = lo.viterbi(e, labs, flags, pen)
        ref = lp.posteriors(e, labs, flags, pen)
        assert r[3] == lo.LA_OK
        seconds.append([None if r[0][n] < 0 else [float(r[0][n]) * HOP, float(r[1][n]) * HOP] for n in range(L)])
        visits = lo.segments(r[4])
        segments.append([(n, float(t) * HOP, float(u) * HOP) for n, t, u in visits])
        occ, onp, offp = lp.scores(ref, r[0], r[1], WINDOW)
        pp = lp.path_prob(ref, r[4])
        dicts.append({"occupancy": list(occ), "onset_prob": list(onp), "offset_prob": list(offp), "path_log_posterior": r[2] - ref["log_z"],
                      "visits": list(ref["visits"]), "visit_occupancy": [float(pp[t:u].mean()) for _, t, u in visits],
                      "line_visits": [ref["visits"][a] for a in line_starts[b]],
                      "line_out_of_order": [ref["visits"][a] - ref["in_order"][a] for a in line_starts[b]]})
    return seconds, segments, dicts


def _scores_close(got, want, T, what):
    assert set(got) == set(want), (what, set(got) ^ set(want))
    tol = bound(T)
    for k, w in want.items():
        g, w = np.asarray(got[k], np.float64), np.asarray(w, np.float64)
        assert g.shape == w.shape, (what, k)
        scale = 2.0 if k == "line_out_of_order" else 1.0                              # the difference of two outputs
        assert (np.abs(g - w) <= scale * tol * np.maximum(1.0, np.abs(w))).all(), (what, k, g, w)


@pytest.mark.parametrize("use_ctc", [True, False])
def test_align_and_the_two_step_route_equal_the_yardstick_on_the_devices_emissions(tiny, use_ctc):
    from lyricalignment_amd import _lib, ops
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels, tr = tiny["model"], tiny["audios"], tiny["labels"], tiny["tr"]
    two = ua.perform_viterbi_ctc_line_confidence if use_ctc else ua.perform_viterbi_line_confidence
    variant = _lib.LA_VARIANT_CTC if use_ctc else _lib.LA_VARIANT_PLAIN
    pen = 0.25
    kw = dict(line_starts=LINE_STARTS, line_jump_penalty=pen)
    with torch.no_grad():
        logits, _ = model.frame_manual_forward(audios)
        lab, n_lab, lists = ua._labels_to_device(labels, 4, logits.device)
        T = logits.shape[1]
        em = ops.emissions_from_logits(logits.float().contiguous(), lab, n_lab, variant).cpu().numpy()
        seconds, segments, dicts = _expected_scores(em, lists, [T] * 4, LINE_STARTS, pen)
        got = two(logits, labels, LINE_STARTS, pen, return_segments=True)
        assert len(got) == 3 and got[0] == seconds and got[1] == segments
        for b in range(4):
            _scores_close(got[2][b], dicts[b], T, ("two-step", b))
        short = two(logits, labels, LINE_STARTS, pen)
        assert len(short) == 2 and short[0] == seconds and short[1] == got[2]
        # the fused head's emissions
        eng = model.engine()
        feats, B, T2, stride = model._features(model._mel_of(audios), True)
        em_head = eng.emissions(feats, B, T2, stride, lab, n_lab, variant).cpu().numpy()
        seconds_h, segments_h, dicts_h = _expected_scores(em_head, lists, [T] * 4, LINE_STARTS, pen)
        fused = model.align(audios, labels, use_ctc=use_ctc, return_segments=True, return_line_confidence=True, **kw)
        assert len(fused) == 3 and fused[0] == seconds_h and fused[1] == segments_h
        for b in range(4):
            _scores_close(fused[2][b], dicts_h[b], T, ("align", b))
        pair = model.align(audios, labels, use_ctc=use_ctc, return_line_confidence=True, **kw)
        assert len(pair) == 2 and pair[0] == seconds_h and pair[1] == fused[2]
        # without the keyword the call is what it was
        assert model.align(audios, labels, use_ctc=use_ctc, return_segments=True, **kw) == (seconds_h, segments_h)
        if use_ctc:                                             # per_clip: every clip as if it ran alone, against the yardstick on its own frames
            batch = model.align(audios, labels, per_clip=True, return_segments=True, return_line_confidence=True, **kw)
            logit_rows = model.frame_logits_per_clip(audios)
            for r, i in enumerate(tiny["idx"]):
                lg = logit_rows[r][None].float().contiguous()
                lab1, n1, lists1 = ua._labels_to_device(tr._clip_labels(i), 1, lg.device)
                em1 = ops.emissions_from_logits(lg, lab1, n1, variant).cpu().numpy()
                s1, g1, d1 = _expected_scores(em1, lists1, [lg.shape[1]], [LINE_STARTS[r]], pen)
                assert batch[0][r] == s1[0] and batch[1][r] == g1[0], i
                _scores_close(batch[2][r], d1[0], lg.shape[1], ("per_clip", i))


def test_align_free_order_scored_on_the_tiny_model(tiny):
    from lyricalignment_amd.harness import PinyinClassLUT, align_free_order, align_free_order_scored
    from test_gpu_parity_full import VOCAB
    model, tr = tiny["model"], tiny["tr"]
    lut = PinyinClassLUT([str(i) for i in range(VOCAB)], {str(i): i for i in range(VOCAB)})           # token id -> the same class id
    ids_all = [int(v) for v in tr._clip_labels(0)[0]]                                                 # 11 labels: lines of 3 / 4 / 2 / 2
    lines = ["".join(chr(0x4E00 + 11 * k + j) for j in range(n)) for k, n in enumerate((3, 4, 2, 2))]
    ids, pos = {}, 0
    for line in lines:
        ids[line] = ids_all[pos: pos + len(line)]
        pos += len(line)
    out = align_free_order_scored(model, tr._clip(0), lines, lut, lambda t: ids[t], line_jump_penalty=0.25)
    plain = align_free_order(model, tr._clip(0), lines, lut, lambda t: ids[t], line_jump_penalty=0.25)
    assert set(out) == set(plain) | {"confidence"} and all(out[k] == plain[k] for k in plain)
    with torch.no_grad():
        _, seg, scores = model.align([tr._clip(0)], tr._clip_labels(0), line_starts=[[0, 3, 7, 9]], line_jump_penalty=0.25, return_segments=True,
                                     return_line_confidence=True)
    conf, d = out["confidence"], scores[0]
    assert set(conf) == {"expected_occurrences", "out_of_order", "occurrence_occupancy", "order_log_posterior"}
    assert conf["expected_occurrences"] == d["line_visits"] and conf["out_of_order"] == d["line_out_of_order"]
    assert conf["order_log_posterior"] == d["path_log_posterior"] <= 1e-6
    assert [len(o) for o in conf["occurrence_occupancy"]] == [len(o) for o in out["occurrences"]]
    flat = [v for occ in conf["occurrence_occupancy"] for v in occ]
    assert all(0.0 <= v <= 1.0 + 1e-5 for v in flat) and len(flat) == len(out["order"])
    # an occurrence's number is the frame-weighted mean of its visits'
    total = sum(v * (u - t) for v, (_, t, u) in zip(d["visit_occupancy"], seg[0]))
    again = sum(v * sum(c[1] - c[0] for c in o) for occ_v, occ in zip(conf["occurrence_occupancy"], out["occurrences"]) for v, o in zip(occ_v, occ))
    assert abs(total - again) <= 1e-9
    assert all(a >= b - 1e-6 for a, b in zip(conf["expected_occurrences"], conf["out_of_order"]))
    print(f"order {out['order']}, expected occurrences {conf['expected_occurrences']}, out of order {conf['out_of_order']}, "
          f"order_log_posterior {conf['order_log_posterior']:.3f}")


# ------------------------------------------------------------------------------------------------ 7. the bench tool
def test_the_bench_tool_runs_quick():
    # --parent-lib: the tree's own library loaded a second time, the control of two loads of one build
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "line_confidence_bench.py"), "--quick", "--parent-lib",
                        os.path.join(ROOT, "lyricalignment_amd", "liblyricalign_hip.so")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    same = [line for line in r.stdout.splitlines() if "same bits as the parent commit's" in line]
    assert same and all(line.endswith(": yes") for line in same), r.stdout
    assert "alignment_posteriors_lines" in r.stdout
