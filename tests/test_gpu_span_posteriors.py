"""la_alignment_posteriors_spans (the SPANS instantiations of csrc/la_posterior.hip) on the GPU against the float64 numpy yardstick
tests/span_posterior_reference.py (pinned to brute-force enumeration by tests/test_host_span_posteriors.py), and the Python surface that
carries the span confidences (ops, AlignModel.align, utils.alignment, harness).

Tolerance: absolute 8 * T * 2**-23 on every probability and on log_z, derived as in tests/test_gpu_posteriors.py -- each of alpha and beta
takes T steps whose three-term log-sum-exp correction is float32 (<= ~2**-23 absolute in the log domain per step), gamma adds the two, the
factor 8 is a two-fold margin for hardware exp / log at 1 ulp.  The jump terms are folded in float64 and add nothing to the per-step budget.
A lattice error (a missing or doubled jump arc, a wrong label rule, an off-by-one source) moves these numbers by 1e-2 to 1.
"""
import json

import numpy as np
import pytest
import torch

import optional_spans_reference as osr
import posterior_reference as pr
import span_posterior_reference as spr

pytestmark = pytest.mark.gpu

SHARED = ("occupancy", "onset_prob", "offset_prob", "log_z", "status")
NAMES = SHARED + ("present_prob", "span_skip_prob")


def _tol(T):
    return 8 * T * 2.0 ** -23


def _pack(ems, labels_list, skips, Tmax=None, Lmax=None):
    B = len(ems)
    Lmax = Lmax or max(max(len(l) for l in labels_list), 1)
    Tmax = Tmax or max(e.shape[0] for e in ems)
    em = torch.zeros((B, Tmax, Lmax + 1), dtype=torch.float32)
    labels = torch.zeros((B, Lmax), dtype=torch.int32)
    skip = torch.full((B, Lmax + 1), -1, dtype=torch.int32)
    for b, (e, l, s) in enumerate(zip(ems, labels_list, skips)):
        em[b, : e.shape[0], : e.shape[1]] = torch.from_numpy(np.ascontiguousarray(e))
        labels[b, : len(l)] = torch.tensor(list(l), dtype=torch.int32)
        skip[b, : len(s)] = torch.tensor(list(s), dtype=torch.int32)
    n_labels = torch.tensor([len(l) for l in labels_list], dtype=torch.int32)
    n_frames = torch.tensor([e.shape[0] for e in ems], dtype=torch.int32)
    return em.cuda(), labels.cuda(), n_labels.cuda(), n_frames.cuda(), skip.cuda()


def _launch(ems, labels_list, skips, penalty, window, want_gamma=True, Tmax=None, Lmax=None):
    """The span DP + the span posteriors in one ragged launch each -> dict of numpy arrays."""
    from lyricalignment_amd import ops
    em, labels, n_labels, n_frames, skip = _pack(ems, labels_list, skips, Tmax, Lmax)
    on, off, score, vstatus = ops.viterbi_spans_batch(em, labels, n_labels, n_frames, skip, penalty)
    res = ops.alignment_posteriors_spans(em, labels, n_labels, n_frames, on, off, skip, penalty, boundary_window=window, want_gamma=want_gamma)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in zip(NAMES + (("gamma",) if want_gamma else ()), res)}
    out.update(onset=on.cpu().numpy(), offset=off.cpu().numpy(), score=score.cpu().numpy(), vstatus=vstatus.cpu().numpy())
    return out


def _compare(r, b, ref, em, lab, skip, window, with_gamma):
    """Clip b of launch r against the yardstick `ref` = spr.posteriors(...) -> {output: max |difference|}, invariants included."""
    T, L = em.shape[0], len(lab)
    S = 2 * L + 1
    gamma_r, entry_r, exit_r, present_r, skip_r, log_z_r = ref
    on, off = r["onset"][b, :L], r["offset"][b, :L]
    occ_r, onp_r, offp_r = spr.scores(gamma_r, entry_r, exit_r, on, off, window)
    present = r["present_prob"][b, :L].astype(np.float64)
    span_skip = r["span_skip_prob"][b, : L + 1].astype(np.float64)
    worst = {"occupancy": np.abs(r["occupancy"][b, :L] - occ_r).max(), "onset_prob": np.abs(r["onset_prob"][b, :L] - onp_r).max(),
             "offset_prob": np.abs(r["offset_prob"][b, :L] - offp_r).max(), "present_prob": np.abs(present - present_r).max(),
             "span_skip_prob": np.abs(span_skip - skip_r).max(), "log_z": abs(r["log_z"][b] - log_z_r),
             "coverage": np.abs(spr.coverage(present, span_skip, skip) - 1).max(),                # the identity, on the device's output
             "path_above_total": max(0.0, r["score"][b] - r["log_z"][b])}
    if with_gamma:
        gamma = r["gamma"][b, :T, :S].astype(np.float64)
        worst["gamma"] = np.abs(gamma - gamma_r).max()                                            # every cell
        worst["gamma_rowsum"] = np.abs(gamma.sum(1) - 1).max()
        worst["gamma_range"] = max(0.0, -gamma.min(), gamma.max() - 1)
    for key in ("occupancy", "onset_prob", "offset_prob", "present_prob", "span_skip_prob"):
        v = r[key][b, : L + (key == "span_skip_prob")].astype(np.float64)
        worst[key + "_range"] = max(0.0, -v.min(), v.max() - 1)
    if window >= T:                              # the whole entry / exit distribution of a reported label is its present_prob
        rep = on >= 0
        if rep.any():
            worst["onset_is_present"] = np.abs(r["onset_prob"][b, :L][rep] - present[rep]).max()
            worst["offset_is_present"] = np.abs(r["offset_prob"][b, :L][rep] - present[rep]).max()
    assert not r["span_skip_prob"][b, [n for n in range(L + 1) if not 0 <= skip[n] < n]].any()    # exactly 0 where no span ends
    assert not (r["occupancy"][b, :L][on < 0].any() or r["onset_prob"][b, :L][on < 0].any() or r["offset_prob"][b, :L][on < 0].any())
    return worst


def _check_clips(cases, name):
    """cases: [(em, labels, skip_from)] -> every clip alone in a launch (max_frames = T, so that window T covers every frame) per penalty,
    window and form; every output against the yardstick, the measured maxima printed before anything is asserted.  Returns the yardstick's
    span_skip values of the declared spans."""
    from lyricalignment_amd import _lib
    forms = [1, 0] if 2 * max(len(c[1]) for c in cases) + 1 <= 64 else [1]
    total, seen, failed = {}, [], []
    for pen in spr.PENALTIES:
        for b, (em, lab, skip) in enumerate(cases):
            T, L = em.shape[0], len(lab)
            ref = spr.posteriors(em, lab, skip, pen)
            seen += [float(ref[4][n]) for _, n in spr.spans_of(skip)]
            r_on, r_off, r_score, r_status, _ = osr.viterbi_spans(em, lab, skip, pen)
            for dpp in forms:
                with _lib.option("viterbi_dpp", dpp):
                    runs = {w: _launch([em], [lab], [skip], pen, w, want_gamma=(w == 2)) for w in (0, 2, T)}
                for w, r in runs.items():
                    assert r["status"][0] == r["vstatus"][0] == r_status == 0, (name, b, pen, w, dpp)
                    assert r["onset"][0, :L].tolist() == r_on and r["offset"][0, :L].tolist() == r_off and r["score"][0] == r_score
                    for k, v in _compare(r, 0, ref, em, lab, skip, w, with_gamma=(w == 2)).items():
                        total[k] = max(total.get(k, 0.0), float(v))
                        if not v <= _tol(T):
                            failed.append((b, pen, w, dpp, k, float(v), _tol(T)))
    T = max(c[0].shape[0] for c in cases)
    print(f"{name}: {len(cases)} clips, forms {forms}, tol(T={T})={_tol(T):.2e}, reference span_skip of the declared spans "
          f"{np.round(sorted(seen), 4).tolist()[:12]}{' ...' if len(seen) > 12 else ''} measured maxima: "
          + json.dumps({k: float(f"{v:.2e}") for k, v in total.items()}))
    assert not failed, (name, failed[:8])
    return seen


# ------------------------------------------------------------------------------------------------ 1. every output against the yardstick
@pytest.mark.parametrize("case", spr.GENERATOR_CASES, ids=lambda c: f"T{c[0]}_lines{len(c[1])}_absent{sorted(c[2])}_lean{c[5]}")
def test_generator_cases_match_reference_and_invariants(case):
    """The four lyric-sheet cases whose spans are certain, impossible and undecided (asserted on the CPU by
    tests/test_host_span_posteriors.py): windows 0, 2 and T, penalties 0 and 1, the DPP and the LDS-exchange form of the one-wave kernel."""
    em, lab, skip = spr.make_inputs(*case)
    _check_clips([(em, lab, skip)], f"sheet T{case[0]} lines {case[1]} absent {sorted(case[2])} lean {case[5]}")


SHAPES = [  # (T, L, what)
    (1, 1, "the only span L = 1 has"), (2, 1, "the only span L = 1 has"), (5, 4, "a repeat inside"),
    (40, 31, "63 states, last one-wave size"), (40, 32, "65 states, first two-wave size"), (120, 100, "four waves"),
    (300, 511, "16 waves, the label limit"),
]


@pytest.mark.parametrize("T,L,what", SHAPES, ids=[f"T{s[0]}_L{s[1]}" for s in SHAPES])
def test_shapes_match_reference_and_invariants(T, L, what):
    """Every size at which the kernel takes another form.  L = 1: the span (0, 1); L = 4: spans around the repeated pair; the larger ones:
    random spans as tests/test_gpu_optional_spans.py builds them (nested, overlapping, sharing starts), lean label columns on the odd clip."""
    import test_gpu_optional_spans as tos
    if L == 1:
        cases = []
        for c in range(2):
            em, lab, skip = tos._random_case(900 + T + c, T, 1, None, n_classes=3, lean=1.5 * c)
            cases.append((em, lab, [-1, 0]))
    elif L == 4:
        cases = []
        for c, spans in enumerate(([(1, 3)], [(0, 2), (2, 4)], [(0, 4), (2, 3)])):
            em, lab, _ = tos._random_case(950 + c, T, 4, 2, n_classes=3, lean=1.5 * (c % 2))
            skip = [-1] * 5
            for a, n in spans:
                skip[n] = a
            cases.append((em, lab, skip))
    else:
        cases = [tos._random_case(31 * T + L + 1000 * c, T, L, L // 2, lean=1.5 * (c % 2)) for c in range(2)]
    seen = _check_clips(cases, f"T{T}_L{L} ({what})")
    if T >= 2 and L > 1:
        assert max(seen) > 1e-3                                      # the jumps carry mass


# ------------------------------------------------------------------------------------------------ 2. no spans
@pytest.mark.parametrize("dpp", [1, 0])
def test_without_spans_equals_alignment_posteriors_bit_for_bit(dpp):
    """Every skip_from entry -1 (and a positive penalty): the five shared outputs and gamma are ops.alignment_posteriors' to the bit,
    present_prob is 1 on the labels and span_skip_prob 0 -- one-wave and multi-wave sizes, an infeasible clip among them."""
    from lyricalignment_amd import _lib, ops
    for specs in ([(60, 9, 1), (33, 31, 2), (4, 4, 3), (17, 3, 4)], [(90, 40, 5), (50, 32, 6)], [(310, 300, 7)]):
        ems, labs = [], []
        for T, L, seed in specs:
            em, lab = pr.make_inputs(T, L, 3.0, seed, flat=(2 * L >= T - 1))
            ems.append(em)
            labs.append(lab)
        em, labels, n_labels, n_frames, skip = _pack(ems, labs, [[-1] * (len(l) + 1) for l in labs])
        with _lib.option("viterbi_dpp", dpp):
            on, off, score, vstatus = ops.viterbi_batch(em, labels, n_labels, n_frames)
            want = ops.alignment_posteriors(em, labels, n_labels, n_frames, on, off, boundary_window=2, want_gamma=True)
            got = ops.alignment_posteriors_spans(em, labels, n_labels, n_frames, on, off, skip, 0.75, boundary_window=2, want_gamma=True)
            torch.cuda.synchronize()
        for name, w, g in zip(SHARED + ("gamma",), want, got[:5] + got[7:]):
            assert w.cpu().numpy().tobytes() == g.cpu().numpy().tobytes(), (specs, name)
        status = got[4].cpu().numpy()
        assert (status == vstatus.cpu().numpy()).all()
        present, span_skip = got[5].cpu().numpy(), got[6].cpu().numpy()
        assert not span_skip.any()
        for b, lab in enumerate(labs):
            assert (present[b, : len(lab)] == (1.0 if status[b] == 0 else 0.0)).all() and not present[b, len(lab):].any()


# ------------------------------------------------------------------------------------------------ 3. one ragged launch
def test_ragged_launch_statuses_zero_rows_and_no_cross_clip_indexing():
    """Mixed T and L in one launch, clips with and without spans, an infeasible and an empty clip: statuses as the DP's, failed rows and rows
    beyond L zero, the others within tolerance of the yardstick; each clip bit-identical to running it alone with the same max_frames and
    max_labels."""
    import test_gpu_optional_spans as tos
    rs = np.random.RandomState(11)
    cases = [tos._random_case(1, 50, 9, 4, lean=1.5), tos._random_case(2, 23, 17, 5)]
    c = tos._random_case(3, 3, 6, None)
    cases.append((c[0], c[1], [-1, -1, 1, -1, -1, -1, -1]))                    # 6 labels, one optional, 3 frames: infeasible
    cases.append((np.zeros((30, 1), np.float32), [], [-1]))                    # empty
    em, lab = pr.make_inputs(200, 31, 3.0, 5)
    cases.append((em, lab, [-1] * 32))                                         # no span
    cases.append(tos._random_case(6, 333, 20, 7, lean=1.5))
    cases.append(spr.make_inputs(40, [2, 2], {1}, 3.0, 7, 6.0))
    cases.append((( -rs.rand(1, 2) * 3).astype(np.float32), [7], [-1, 0]))
    ems, labs, skips = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    Tmax, Lmax = 333, 31
    for pen, w in ((0.0, 2), (1.0, 0)):
        r = _launch(ems, labs, skips, pen, w)
        assert r["status"].tolist() == r["vstatus"].tolist() == [0, 0, 2, 3, 0, 0, 0, 0]
        assert r["gamma"].shape == (len(cases), Tmax, 2 * Lmax + 1) and r["span_skip_prob"].shape == (len(cases), Lmax + 1)
        for b, (em, lab, skip) in enumerate(cases):
            T, L = em.shape[0], len(lab)
            S = 2 * L + 1
            for key in ("occupancy", "onset_prob", "offset_prob", "present_prob"):
                assert not r[key][b, L:].any(), (b, key)
            assert not r["span_skip_prob"][b, L + 1:].any()
            assert not r["gamma"][b, T:].any() and not r["gamma"][b, :, S:].any()
            if r["status"][b] != 0:
                for key in ("gamma", "occupancy", "onset_prob", "offset_prob", "present_prob", "span_skip_prob"):
                    assert not r[key][b].any(), (b, key)
                assert r["log_z"][b] == (-np.inf if r["status"][b] == 2 else 0.0)
            else:
                worst = _compare(r, b, spr.posteriors(em, lab, skip, pen), em, lab, skip, w, with_gamma=True)
                print(f"ragged penalty={pen} w={w} b={b} T={T} L={L} tol={_tol(T):.2e}: " + json.dumps({k: float(f"{v:.2e}") for k, v in worst.items()}))
                for k, v in worst.items():
                    assert v <= _tol(T), (b, k, v)
            alone = _launch([em], [lab], [skip], pen, w, Tmax=Tmax, Lmax=Lmax)
            for key in NAMES + ("gamma",):
                assert alone[key][0].tobytes() == r[key][b].tobytes(), (b, key)


def test_ops_wrapper_rejects_bad_arguments():
    from lyricalignment_amd import ops
    em = torch.zeros((2, 10, 5), dtype=torch.float32).cuda()
    lab = torch.ones((2, 4), dtype=torch.int32).cuda()
    n = torch.tensor([4, 4], dtype=torch.int32).cuda()
    t = torch.tensor([10, 10], dtype=torch.int32).cuda()
    skip = torch.full((2, 5), -1, dtype=torch.int32).cuda()
    on = torch.zeros((2, 4), dtype=torch.int32).cuda()
    for bad in (dict(skip_from=skip[:, :4]), dict(skip_from=skip.long()), dict(skip_penalty=-1.0), dict(skip_penalty=float("nan")),
                dict(boundary_window=-1)):
        kw = dict(skip_from=skip, skip_penalty=0.0, boundary_window=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.alignment_posteriors_spans(em, lab, n, t, on, on, **kw)
    with pytest.raises(NotImplementedError):
        z = torch.zeros((1, 8, 513), dtype=torch.float32, device="cuda")
        i = torch.zeros((1, 512), dtype=torch.int32, device="cuda")
        one = torch.ones((1,), dtype=torch.int32, device="cuda")
        ops.alignment_posteriors_spans(z, i, one, one * 8, i, i, torch.full((1, 513), -1, dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------------------------------------ 4. the Python surface on the tiny model
IDX = [0, 1, 3, 5]                                           # clips of tests/test_gpu_ragged.py: 11, 5, 8, 3 labels
SPANS = [[(3, 7), (0, 3)], [(3, 5)], [(2, 5)], []]           # (clip 0: given out of order on purpose)
SCORE_KEYS = ("occupancy", "onset_prob", "offset_prob", "sung_prob", "span_skip_prob")


@pytest.fixture(scope="module")
def tiny():
    import test_gpu_ragged as tr
    from test_gpu_parity_full import _build
    model, _ = _build("tiny", torch.float32)
    return dict(model=model, audios=[tr._clip(i) for i in IDX], labels=tr._padded_labels(IDX), tr=tr)


def _scores_close(got, want, tol, what):
    worst = 0.0
    assert set(got) == set(want) == set(SCORE_KEYS) | {"path_log_posterior"}, what
    for key in SCORE_KEYS:
        assert len(got[key]) == len(want[key]), (what, key)
        assert all(isinstance(v, float) for v in got[key])
        if len(want[key]):
            worst = max(worst, float(np.abs(np.asarray(got[key]) - np.asarray(want[key])).max()))
    worst = max(worst, abs(got["path_log_posterior"] - want["path_log_posterior"]))
    print(f"{what}: max |difference| {worst:.2e} (tol {tol:.2e})")
    assert worst <= tol, (what, worst, tol)


def _skip_rows(spans, L):
    row = [-1] * (L + 1)
    for a, n in spans:
        row[n] = a
    return row


@pytest.mark.parametrize("use_ctc", [True, False])
def test_span_confidence_through_align_equals_the_yardstick_on_the_engines_emissions(tiny, use_ctc):
    from lyricalignment_amd import _lib
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels = tiny["model"], tiny["audios"], tiny["labels"]
    eng = model.engine()
    lists = ua._label_lists(labels, len(audios))
    variant = _lib.LA_VARIANT_CTC if use_ctc else _lib.LA_VARIANT_PLAIN
    with torch.no_grad():
        mel = model._mel_of(audios)
        feats, B, T, stride = model._features(mel.to(eng.device), True)
        lab_dev, n_lab, _ = ua._labels_to_device(labels, B, eng.device)
        em = eng.align_feats(feats, B, T, stride, lab_dev, n_lab, variant, want_emissions=True)[4].cpu().numpy()
        eng.check_gru()
        logits, _ = model.frame_manual_forward(audios)
        for pen, w in ((0.0, 2), (2.0, 0)):
            what = f"use_ctc={use_ctc} penalty={pen} w={w}"
            plain = model.align(audios, labels, use_ctc=use_ctc, optional_spans=SPANS, skip_penalty=pen)
            seconds, scores = model.align(audios, labels, use_ctc=use_ctc, optional_spans=SPANS, skip_penalty=pen,
                                          return_span_confidence=True, boundary_window=w)
            assert seconds == plain, what
            frames = model.align(audios, labels, use_ctc=use_ctc, optional_spans=SPANS, skip_penalty=pen, return_span_confidence=True,
                                 boundary_window=w, return_frames=True)
            assert len(frames) == 10 and all(torch.is_tensor(t) and t.is_cuda for t in frames)
            assert frames[3].tolist() == [0] * 4 and frames[8].shape == lab_dev.shape and frames[9].shape == (B, lab_dev.shape[1] + 1)
            for b in range(B):
                L = len(lists[b])
                on, off = frames[0][b, :L].cpu().numpy(), frames[1][b, :L].cpu().numpy()
                assert [None if v < 0 else v for v in on.tolist()] == [None if r is None else round(r[0] / 0.02) for r in seconds[b]]
                skip = _skip_rows(SPANS[b], L)
                gamma_r, entry_r, exit_r, present_r, skip_r, log_z_r = spr.posteriors(em[b][:, : L + 1], lists[b], skip, pen)
                occ, onp, offp = spr.scores(gamma_r, entry_r, exit_r, on, off, w)
                want = {"occupancy": occ.tolist(), "onset_prob": onp.tolist(), "offset_prob": offp.tolist(), "sung_prob": present_r.tolist(),
                        "span_skip_prob": [float(skip_r[n]) for _, n in SPANS[b]], "path_log_posterior": float(frames[2][b]) - float(log_z_r)}
                _scores_close(scores[b], want, _tol(T), f"{what} clip {b}")
                assert [float(v) for v in frames[8][b, :L].cpu().numpy()] == scores[b]["sung_prob"]
                assert all(0.0 <= v <= 1 + _tol(T) for key in SCORE_KEYS for v in scores[b][key]) and scores[b]["path_log_posterior"] <= _tol(T)
            print(f"{what}: skipped labels per clip {[sum(r is None for r in res) for res in seconds]}, span_skip_prob "
                  f"{[np.round(s['span_skip_prob'], 4).tolist() for s in scores]}")
            # the two-step drop-in on materialised logits
            two = ua.perform_viterbi_ctc_scored if use_ctc else ua.perform_viterbi_scored
            res2, sc2 = two(logits, labels, boundary_window=w, optional_spans=SPANS, skip_penalty=pen)
            assert res2 == seconds, what
            for b in range(B):
                _scores_close(sc2[b], scores[b], _tol(T), f"{what} two-step clip {b}")
        # no span at all: return_confidence's numbers, sung_prob 1, no span_skip_prob; the scored two-step functions keep their dicts
        sec_c, sc_c = model.align(audios, labels, use_ctc=use_ctc, return_confidence=True)
        for spans in (None, [[], [], [], []]):
            sec_s, sc_s = model.align(audios, labels, use_ctc=use_ctc, optional_spans=spans, return_span_confidence=True)
            assert sec_s == sec_c
            for b in range(B):
                assert sc_s[b]["span_skip_prob"] == [] and np.abs(np.asarray(sc_s[b]["sung_prob"]) - 1).max() <= _tol(T)
                assert {k: v for k, v in sc_s[b].items() if k not in ("sung_prob", "span_skip_prob")} == sc_c[b]
        two = ua.perform_viterbi_ctc_scored if use_ctc else ua.perform_viterbi_scored
        assert set(two(logits, labels)[1][0]) == set(two(logits, labels, optional_spans=[[], [], [], []])[1][0]) == {
            "occupancy", "onset_prob", "offset_prob", "path_log_posterior"}


def test_per_clip_and_long_form_with_span_confidence_and_the_refusals(tiny):
    from lyricalignment_amd import ops
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels, tr = tiny["model"], tiny["audios"], tiny["labels"], tiny["tr"]
    with torch.no_grad():
        seconds, scores = model.align(audios, labels, per_clip=True, optional_spans=SPANS, skip_penalty=0.5, return_span_confidence=True)
        assert seconds == model.align(audios, labels, per_clip=True, optional_spans=SPANS, skip_penalty=0.5)
        for r, i in enumerate(IDX):
            alone = model.align([audios[r]], tr._clip_labels(i), per_clip=True, optional_spans=[SPANS[r]], skip_penalty=0.5,
                                return_span_confidence=True)
            assert seconds[r] == alone[0][0], i
            # a batch of one runs other GEMM tiles: its emissions differ in their last bits, the scores by far less than the 0.1 to 1 of
            # a clip that got another clip's rows, frame count or span list
            _scores_close(scores[r], alone[1][0], 1e-2, f"per_clip clip {i} in the batch against alone")
        # long form: a 33 s recording (two encoder chunks, 1650 frames), 14 labels in four lines, two of them optional
        audio = np.concatenate([tr._clip(4), tr._clip(3)])
        lab14 = torch.from_numpy(np.random.RandomState(5).randint(2, 403, size=(1, 14)))
        spans = [[(3, 7), (10, 14)]]
        logits, _ = model.frame_manual_forward([audio])
        assert logits.shape[1] > 1500
        sec_l, sc_l = model.align([audio], lab14, optional_spans=spans, return_span_confidence=True)
        sec_2, sc_2 = ua.perform_viterbi_ctc_scored(logits, lab14, optional_spans=spans)
        assert sec_l == sec_2 == model.align([audio], lab14, optional_spans=spans)
        _scores_close(sc_l[0], sc_2[0], _tol(logits.shape[1]), "long form against the two-step route")
        cov = np.asarray(sc_l[0]["sung_prob"])
        for (a, n), v in zip(spans[0], sc_l[0]["span_skip_prob"]):
            cov[a:n] += v
        assert np.abs(cov - 1).max() <= _tol(logits.shape[1])
        # refusals
        with pytest.raises(ValueError):
            model.align(audios, labels, optional_spans=SPANS, return_confidence=True)
        with pytest.raises(ValueError):
            model.align(audios, labels, optional_spans=SPANS, return_confidence=True, return_span_confidence=True)
        with pytest.raises(ValueError):
            model.align(audios, labels, optional_spans=SPANS, skip_penalty=-1.0, return_span_confidence=True)
        with pytest.raises(ValueError):
            model.align(audios, labels, skip_penalty=-1.0, return_span_confidence=True)
        with pytest.raises(NotImplementedError):
            many = torch.from_numpy(np.random.RandomState(6).randint(2, 403, size=(1, 512)))
            model.align([tr._clip(4)], many, optional_spans=[[(0, 2)]], return_span_confidence=True)


def test_align_record_lines_with_confidence_returns_none_lines_with_their_sung_probability(tiny):
    from lyricalignment_amd.harness import PinyinClassLUT, align_record_lines
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
    spans = [[(0, 3), (3, 7), (9, 11)]]
    starts = [0, 3, 7, 9]
    tol = _tol(tr.TS[0])
    left_out = 0
    for pen in (0.0, 3.0):
        plain = align_record_lines(model, tr._clip(0), lines, optional, lut, lambda t: ids[t], use_ctc_loss=True, skip_penalty=pen)
        got, sung = align_record_lines(model, tr._clip(0), lines, optional, lut, lambda t: ids[t], use_ctc_loss=True, skip_penalty=pen,
                                       with_confidence=True)
        assert got == plain and len(sung) == 4 and all(isinstance(v, float) for v in sung)
        with torch.no_grad():
            scores = model.align([tr._clip(0)], tr._clip_labels(0), use_ctc=True, optional_spans=spans, skip_penalty=pen,
                                 return_span_confidence=True)[1][0]
        assert sung == [scores["sung_prob"][s] for s in starts]
        assert abs(sung[2] - 1) <= tol and got[2] is not None                       # the mandatory line
        for i, k in ((0, 0), (1, 1), (3, 2)):                                       # an optional line under no other span: 1 - its span's mass
            assert abs(sung[i] - (1 - scores["span_skip_prob"][k])) <= tol
            assert 0.0 <= sung[i] <= 1 + tol
        left_out += sum(e is None for e in got)
        print(f"penalty {pen}: lines left out {[i for i, e in enumerate(got) if e is None]}, sung {np.round(sung, 4).tolist()}")
    assert left_out > 0                                                             # None lines come with their sung values
