"""la_alignment_posteriors (csrc/la_posterior.hip) on the GPU against the float64 numpy yardstick
(tests/posterior_reference.py, itself pinned to brute-force enumeration by tests/test_host_posteriors.py), and the
Python surface that carries the confidences (ops, engine, AlignModel.align, utils.alignment, harness).

Tolerance, derived and not tuned: absolute 8 * T * 2**-23 on every probability and on log_z.  Each of alpha and beta
takes T steps; a step whose log-sum-exp correction is float32 errs by at most about 2**-23 absolute in the log domain;
gamma adds the two; the factor 8 is a two-fold margin for hardware exp / log that round to 1 ulp rather than half.
A lattice error (wrong skip rule, off-by-one window, missing end state) moves these numbers by 1e-2 to 1.
"""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import posterior_reference as pr
from conftest import e2e_cases

pytestmark = pytest.mark.gpu


def _tol(T):
    return 8 * T * 2.0 ** -23


def _pack(ems, labels_list, Tmax=None, Lmax=None):
    B = len(ems)
    Lmax = Lmax or max(max(len(l) for l in labels_list), 1)
    Tmax = Tmax or max(e.shape[0] for e in ems)
    em = torch.zeros((B, Tmax, Lmax + 1), dtype=torch.float32)
    labels = torch.zeros((B, Lmax), dtype=torch.int32)
    for b, (e, l) in enumerate(zip(ems, labels_list)):
        em[b, : e.shape[0], : e.shape[1]] = torch.from_numpy(np.ascontiguousarray(e))
        labels[b, : len(l)] = torch.tensor(list(l), dtype=torch.int32)
    n_labels = torch.tensor([len(l) for l in labels_list], dtype=torch.int32)
    n_frames = torch.tensor([e.shape[0] for e in ems], dtype=torch.int32)
    return em.cuda(), labels.cuda(), n_labels.cuda(), n_frames.cuda()


def _launch(ems, labels_list, window, want_gamma=True, Tmax=None, Lmax=None):
    """DP + posteriors in one ragged launch each -> dict of numpy arrays."""
    from lyricalignment_amd import ops
    em, labels, n_labels, n_frames = _pack(ems, labels_list, Tmax, Lmax)
    on, off, score, vstatus = ops.viterbi_batch(em, labels, n_labels, n_frames)
    res = ops.alignment_posteriors(em, labels, n_labels, n_frames, on, off, boundary_window=window, want_gamma=want_gamma)
    torch.cuda.synchronize()
    names = ("occupancy", "onset_prob", "offset_prob", "log_z", "status") + (("gamma",) if want_gamma else ())
    out = {k: v.cpu().numpy() for k, v in zip(names, res)}
    out.update(onset=on.cpu().numpy(), offset=off.cpu().numpy(), score=score.cpu().numpy(), vstatus=vstatus.cpu().numpy())
    return out


def _check_case(em, lab, name):
    """Items 3 and 4 of the feature's checks on one utterance: every output against the yardstick, then the invariants."""
    T, L = em.shape[0], len(lab)
    S = 2 * L + 1
    tol = _tol(T)
    gamma_r, entry_r, exit_r, log_z_r = pr.posteriors(em, lab)
    runs = {w: _launch([em], [lab], w, want_gamma=(w == 2)) for w in (0, 2, T)}
    on, off = runs[2]["onset"][0, :L], runs[2]["offset"][0, :L]
    assert runs[2]["vstatus"][0] == 0 and (on >= 0).all()
    worst = {}
    for w, r in runs.items():
        assert r["status"][0] == 0
        assert (r["onset"] == runs[2]["onset"]).all() and (r["offset"] == runs[2]["offset"]).all()
        occ_r, onp_r, offp_r = pr.scores(gamma_r, entry_r, exit_r, on, off, w)
        for key, ref in (("occupancy", occ_r), ("onset_prob", onp_r), ("offset_prob", offp_r)):
            worst[f"{key}[w={w}]"] = np.abs(r[key][0, :L].astype(np.float64) - ref).max()
        worst[f"log_z[w={w}]"] = abs(r["log_z"][0] - log_z_r)
    gamma = runs[2]["gamma"][0].astype(np.float64)
    assert gamma.shape == (T, S)
    worst["gamma"] = np.abs(gamma - gamma_r).max()                     # every cell, nothing left out
    worst["gamma_rowsum"] = np.abs(gamma.sum(1) - 1).max()
    occ_r = pr.scores(gamma_r, entry_r, exit_r, on, off, 2)[0]
    print(f"{name}: T={T} L={L} tol={tol:.2e} reference occupancy {occ_r.min():.3f}..{occ_r.max():.3f} "
          f"path_log_posterior {runs[2]['score'][0] - runs[2]['log_z'][0]:.3f} measured maxima: "
          + json.dumps({k: float(f"{v:.2e}") for k, v in worst.items()}))
    for k, v in worst.items():
        assert v <= tol, (name, k, v, tol)
    # invariants, at the same tolerance (they inherit the sweeps' error)
    for w, r in runs.items():
        for key in ("occupancy", "onset_prob", "offset_prob"):
            v = r[key][0, :L]
            assert (v >= 0).all() and (v <= 1 + tol).all(), (name, key, w)
    assert (gamma >= 0).all() and (gamma <= 1 + tol).all()
    assert np.abs(runs[T]["onset_prob"][0, :L] - 1).max() <= tol and np.abs(runs[T]["offset_prob"][0, :L] - 1).max() <= tol
    assert (runs[2]["onset_prob"][0, :L] >= runs[0]["onset_prob"][0, :L]).all()
    assert (runs[2]["offset_prob"][0, :L] >= runs[0]["offset_prob"][0, :L]).all()
    assert runs[2]["score"][0] - runs[2]["log_z"][0] <= tol
    return worst


CASES = [(1500, 26, 12.0, 1, False), (1500, 26, 35.0, 2, False), (400, 19, 3.0, 3, False), (5389, 171, 12.0, 4, False),
         (9000, 238, 0.05, 5, False), (700, 40, 12.0, 6, False), (600, 500, 0.05, 7, True)]


@pytest.mark.parametrize("T,L,scale,seed,flat", CASES, ids=lambda v: str(v))
def test_kernel_matches_reference_and_invariants(T, L, scale, seed, flat):
    """One wave (S <= 64, DPP shifts) and the multi-wave LDS form up to its last supported size (S = 1001)."""
    em, lab = pr.make_inputs(T, L, scale, seed, flat)
    _check_case(em, lab, f"synthetic T{T}_L{L}_s{scale}")


def test_kernel_matches_reference_on_reference_generated_emissions():
    """The emissions the reference fed its DP (tests/golden/viterbi_e2e.npz)."""
    n = 0
    for m, b, em, label, _ in e2e_cases():
        _check_case(np.ascontiguousarray(em, dtype=np.float32), [int(v) for v in label], f"golden {m['name']}/{b}")
        n += 1
    assert n > 0


def test_single_wave_lds_form_matches_reference():
    """Option viterbi_dpp = 0 pins the LDS-exchange form for S <= 64 as well (the A/B partner of the DPP form)."""
    from lyricalignment_amd import _lib
    em, lab = pr.make_inputs(1500, 26, 12.0, 1)
    with _lib.option("viterbi_dpp", 0):
        _check_case(em, lab, "synthetic T1500_L26 LDS form")


def test_ragged_launch_statuses_zero_rows_and_no_cross_utterance_indexing():
    """Ragged T and L in one launch, with an infeasible and an empty utterance: statuses as the DP's, failed rows and rows
    n >= L_b zero, the others within tolerance of the yardstick; each utterance bit-identical to running it alone in a launch
    with the same max_frames and max_labels."""
    rs = np.random.RandomState(7)
    specs = [(50, 3), (5, 4), (4, 4), (200, 31), (1, 1), (30, 0), (333, 17), (2, 1)]
    ems, labs = [], []
    for T, L in specs:
        ems.append((-rs.rand(T, L + 1) * 3).astype(np.float32))
        lab = rs.randint(1, 400, size=L)
        if L == 4:
            lab[2] = lab[1]                     # the repeat needs one extra frame: T = 4 infeasible, T = 5 feasible
        pr.fix_repeats(ems[-1], lab)
        labs.append([int(v) for v in lab])
    Tmax, Lmax = 333, 31
    keys = ("occupancy", "onset_prob", "offset_prob", "log_z", "status", "gamma")
    for w in (0, 2):
        r = _launch(ems, labs, w)
        assert r["status"].tolist() == r["vstatus"].tolist() == [0, 0, 2, 0, 0, 3, 0, 0]
        assert r["gamma"].shape == (len(specs), Tmax, 2 * Lmax + 1)
        for b, (T, L) in enumerate(specs):
            S = 2 * L + 1
            for key in ("occupancy", "onset_prob", "offset_prob"):
                assert not r[key][b, L:].any(), (b, key)
            assert not r["gamma"][b, T:].any() and not r["gamma"][b, :, S:].any()
            if r["status"][b] != 0:
                assert not r["gamma"][b].any() and not r["occupancy"][b].any() and not r["onset_prob"][b].any() and not r["offset_prob"][b].any()
                assert r["log_z"][b] == (-np.inf if r["status"][b] == 2 else 0.0)
            else:
                tol = _tol(T)
                gamma_r, entry_r, exit_r, log_z_r = pr.posteriors(ems[b], labs[b])
                occ_r, onp_r, offp_r = pr.scores(gamma_r, entry_r, exit_r, r["onset"][b, :L], r["offset"][b, :L], w)
                worst = {"gamma": np.abs(r["gamma"][b, :T, :S] - gamma_r).max(), "log_z": abs(r["log_z"][b] - log_z_r),
                         "occupancy": np.abs(r["occupancy"][b, :L] - occ_r).max(), "onset_prob": np.abs(r["onset_prob"][b, :L] - onp_r).max(),
                         "offset_prob": np.abs(r["offset_prob"][b, :L] - offp_r).max()}
                print(f"ragged w={w} b={b} T={T} L={L} tol={tol:.2e}: " + json.dumps({k: float(f"{v:.2e}") for k, v in worst.items()}))
                for k, v in worst.items():
                    assert v <= tol, (b, k, v, tol)
            alone = _launch([ems[b]], [labs[b]], w, Tmax=Tmax, Lmax=Lmax)
            for key in keys:
                assert np.array_equal(alone[key][0], r[key][b]), (b, key)


# ------------------------------------------------------------------------------------------------ surface
def _wave(n, seed=0):
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    return (rs.randn(n) * 0.05 + 0.3 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 3000 * t * (1 + 0.1 * t))).astype(np.float32)


def _model(dtype=torch.float32, seed=0, vocab=300, dropout=0.15):
    from lyricalignment_amd import whisper_compat as wc
    from lyricalignment_amd.module.align_model import AlignModel
    dims = wc.ModelDimensions(n_audio_state=128, n_audio_head=2, n_audio_layer=2, n_text_state=128, n_text_head=2, n_text_layer=1,
                              n_vocab=311, n_text_ctx=64)
    wm = wc.build_model(dims=dims, seed=seed, std=0.05, with_decoder=False)
    model = AlignModel(wm, embed_dim=128, hidden_dim=64, output_dim=vocab, dropout=dropout, device="cuda", compute_dtype=dtype)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in model.align_rnn.named_parameters():
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * ((6.0 if n.startswith("fc.weight") else 1.5) / 64 ** 0.5))
    return model.eval()


def _scores_close(got, want, tol, what):
    worst = 0.0
    for key in ("occupancy", "onset_prob", "offset_prob"):
        assert len(got[key]) == len(want[key]), (what, key)
        assert all(isinstance(v, float) for v in got[key])
        if len(want[key]):
            worst = max(worst, float(np.abs(np.asarray(got[key]) - np.asarray(want[key])).max()))
    assert isinstance(got["path_log_posterior"], float)
    worst = max(worst, abs(got["path_log_posterior"] - want["path_log_posterior"]))
    print(f"{what}: max |difference| {worst:.2e} (tol {tol:.2e})")
    assert worst <= tol, (what, worst, tol)


def _reference_scores(em, lab, on, off, score, w):
    gamma_r, entry_r, exit_r, log_z_r = pr.posteriors(em, lab)
    occ, onp, offp = pr.scores(gamma_r, entry_r, exit_r, on, off, w)
    return {"occupancy": occ.tolist(), "onset_prob": onp.tolist(), "offset_prob": offp.tolist(), "path_log_posterior": float(score - log_z_r)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_confidence_through_the_python_surface(dtype, monkeypatch):
    """AlignModel.align(return_confidence=True), engine.align_feats(want_emissions=True), perform_viterbi_ctc_scored and
    harness.align_records(with_confidence=True) on a small random-weight model, on both head routes (the C call and the
    op-by-op sequencing).  The scores are compared with the yardstick evaluated on the engine's OWN emissions for that batch:
    that isolates the plumbing from the encoder's dtype error."""
    from lyricalignment_amd import engine as eng_mod, harness
    from lyricalignment_amd.utils.alignment import _labels_to_device, perform_viterbi_ctc, perform_viterbi_ctc_scored
    model = _model(dtype, seed=120)
    eng = model.engine()
    audios = [_wave(16000 * 31 + 480, 121), _wave(16000 * 12, 122), _wave(16000 * 20 + 77, 123)]     # the first is long-form: > 3000 mel frames
    labels = [[5, 17, 17, 250, 9, 33, 120, 7, 64], [44, 3, 298, 12], [8, 8, 191, 23, 60, 2]]
    short = [_wave(16000 * 6, 124), _wave(16000 * 4 + 160, 125)]
    short_labels = [[21, 90, 90], [7, 150, 33, 4, 18]]
    for route_py in (False, True):
        monkeypatch.setattr(eng_mod, "ENGINE_PY", route_py)
        for clips, labs, orig_len, w in ((audios, labels, True, 2), (short, short_labels, True, 0), (short, short_labels, False, 2)):
            what = f"{'op-by-op' if route_py else 'C call'} {len(clips)} clips get_orig_len={orig_len} w={w}"
            plain = model.align(clips, labs, get_orig_len=orig_len)
            seconds, scores = model.align(clips, labs, get_orig_len=orig_len, return_confidence=True, boundary_window=w)
            assert seconds == plain, what
            assert len(scores) == len(clips)
            # the engine's own emissions for this batch
            with torch.no_grad():
                mel = model._mel_of(clips)
                feats, B, T, stride = model._features(mel.to(eng.device), orig_len)
                lab_dev, n_lab, lists = _labels_to_device(labs, B, eng.device)
                on, off, score, status, em = eng.align_feats(feats, B, T, stride, lab_dev, n_lab, 1, want_emissions=True)
                four = eng.align_feats(feats, B, T, stride, lab_dev, n_lab, 1)
            eng.check_gru()
            assert len(four) == 4 and all(torch.equal(a, b) for a, b in zip(four, (on, off, score, status)))
            assert em.shape == (B, T, max(map(len, labs)) + 1) and em.dtype == torch.float32
            if clips is audios:
                assert mel.shape[-1] > 3000 and T > 1500
            assert int(status.abs().sum()) == 0
            for b in range(B):
                L = len(labs[b])
                assert seconds[b] == [[float(int(a)) * 0.02, float(int(c)) * 0.02] for a, c in zip(on[b, :L].tolist(), off[b, :L].tolist())]
                want = _reference_scores(em[b].cpu().numpy(), labs[b], on[b, :L].cpu().numpy(), off[b, :L].cpu().numpy(), float(score[b]), w)
                _scores_close(scores[b], want, _tol(T), f"{what} clip {b}")
                assert min(scores[b]["occupancy"]) >= 0 and max(scores[b]["occupancy"]) <= 1 + _tol(T)
                assert scores[b]["path_log_posterior"] <= _tol(T)
            frames = model.align(clips, labs, get_orig_len=orig_len, return_confidence=True, boundary_window=w, return_frames=True)
            assert len(frames) == 8 and all(torch.is_tensor(t) and t.is_cuda for t in frames)
            assert torch.equal(frames[0], on) and torch.equal(frames[1], off)
            for b in range(B):
                L = len(labs[b])
                assert [float(v) for v in frames[4][b, :L].cpu().numpy()] == scores[b]["occupancy"]
                assert not frames[4][b, L:].any()
        # two-step drop-in: logits -> perform_viterbi_ctc_scored
        clip, lab = short[0], torch.tensor([short_labels[0]])
        with torch.no_grad():
            logits, _ = model.frame_manual_forward([clip])
        res, sc = perform_viterbi_ctc_scored(logits, lab)
        assert res == perform_viterbi_ctc(logits, lab)
        res_cpu, sc_cpu = perform_viterbi_ctc_scored(logits.cpu(), lab, boundary_window=2)
        assert res_cpu == res and sc_cpu == sc
        seconds, scores = model.align([clip], lab, return_confidence=True)
        assert seconds == res
        _scores_close(sc[0], scores[0], _tol(logits.shape[1]), f"{'op-by-op' if route_py else 'C call'} two-step against align")
        # harness
        lut = harness.PinyinClassLUT([f"p{i}" for i in range(26)], {f"p{i}": 10 + 3 * i for i in range(26)})
        records = [SimpleNamespace(text="abca", audio=short[0]), SimpleNamespace(text="zq", audio=short[1])]
        tokenize = lambda text: [ord(c) - 97 for c in text]
        rows3 = harness.align_records(model, records, lut, tokenize)
        rows4 = harness.align_records(model, records, lut, tokenize, with_confidence=True)
        for rec, r3, r4 in zip(records, rows3, rows4):
            assert len(r4) == len(rec.text) and all(len(e) == 4 for e in r4) and all(len(e) == 3 for e in r3)
            assert [e[:3] for e in r4] == r3
            want = model.align([rec.audio], lut(torch.tensor([tokenize(rec.text)])), return_confidence=True)[1][0]["occupancy"]
            assert [e[3] for e in r4] == want and all(0.0 <= v <= 1 + _tol(1500) for v in want)


def test_error_types_of_the_scored_functions_match_the_unscored_ones():
    """Same exception types as perform_viterbi_ctc: ValueError for an infeasible utterance, IndexError for an empty one."""
    from lyricalignment_amd.utils.alignment import perform_viterbi_ctc, perform_viterbi_ctc_scored, perform_viterbi_scored
    logits = torch.from_numpy(np.random.RandomState(3).randn(1, 4, 40).astype(np.float32))
    for fn in (perform_viterbi_ctc, perform_viterbi_ctc_scored, perform_viterbi_scored):
        with pytest.raises(ValueError, match="is not in list"):
            fn(logits, torch.tensor([[3, 5, 5, 7]]))
        with pytest.raises(IndexError):
            fn(logits, torch.tensor([[-100, -100]]))
    with pytest.raises(NotImplementedError):
        from lyricalignment_amd import ops
        z = torch.zeros((1, 8, 513), dtype=torch.float32, device="cuda")
        i = torch.zeros((1, 512), dtype=torch.int32, device="cuda")
        one = torch.ones((1,), dtype=torch.int32, device="cuda")
        ops.alignment_posteriors(z, i, one, one * 8, i, i)
