"""The float64 restatement of la_multitask_loss (tests/loss_reference.py) pinned to float64 torch autograd wherever torch defines the case,
the cases torch does not define checked against the header's statement, the float32 yardstick e32 checked not to fold a row's maximum
into its log-sum, and the host-side argument checks of the entry and of its workspace query.  Runs without a GPU."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import loss_reference as LR

# Two float64 evaluations of the same quantity, measured with rel_err (max |a - ref| / max(|ref|, 1)) like every pin of
# tests/test_host_row_kernels.py.  Relative to the gradient's largest entry the restatement stays below 1e-12 of float64 torch on every
# case but the 511-label one (530 frames, path scores near -2000, where one ulp of a score is 2.3e-13): 1.6e-12 there, and float64 torch
# itself lies 2.4e-12 from the same sweep carried out in 80-bit floats.  The test prints both figures.
TIGHT = 1e-12


def _torch_terms(c):
    """float64 torch: (ce, bce, ctc) as scalars on a leaf x; a term torch cannot evaluate for the case is None."""
    V, T, B = c["V"], c["T"], c["B"]
    x = c["x"].double().requires_grad_(True)
    fl = c["fl"].long()
    ce = None
    if c["frames"] != "all_ignored":
        tgt = torch.where((fl >= 1) & (fl < V), fl - 1, torch.full_like(fl, -100))      # labels shifted by one onto columns 1..V-1
        ce = F.cross_entropy(x[:, :, 1:V].transpose(1, 2), tgt, ignore_index=-100)
    bce = F.binary_cross_entropy_with_logits(x[:, :, V], (fl == -100).double())
    ctc = None
    if all(LR.clip_state(c, b) == "ok" for b in range(B)):
        lsm = F.log_softmax(x[:, :, :V], dim=2).transpose(0, 1)
        ctc = F.ctc_loss(lsm, c["lab"].long(), torch.full((B,), T, dtype=torch.long), c["n_labels"].long(), blank=0, reduction="mean")
    return x, ce, bce, ctc


@pytest.mark.parametrize("name", LR.CASE_NAMES)
def test_restatement_matches_float64_torch_autograd(name):
    c = LR.make(name)
    x, ce, bce, ctc = _torch_terms(c)
    modes = ([] if ce is None else ["ce"]) + ([] if ctc is None else ["ctc"]) + ([] if ce is None or ctc is None else ["both"])
    assert modes or c["special"]
    for mode in modes:
        use_ce, use_ctc, scale = LR.MODES[mode]
        losses, nll, d = LR.losses_and_grad(c["x"], c["fl"], c["lab"], c["n_labels"], c["V"], scale, use_ce, use_ctc)
        total = (ce + bce if use_ce else 0) + (ctc if use_ctc else 0)
        x.grad = None
        (scale * total).backward(retain_graph=True)
        if use_ce:
            assert LR.rel_err(losses[0], ce) <= TIGHT and LR.rel_err(losses[1], bce) <= TIGHT
        if use_ctc:
            assert LR.rel_err(losses[2], ctc) <= TIGHT, (float(losses[2]), float(ctc.detach()))
            mean = sum(float(nll[b]) / int(c["n_labels"][b]) for b in range(c["B"])) / c["B"]
            assert abs(mean - float(ctc.detach())) <= TIGHT * max(1.0, abs(float(ctc.detach())))
        assert d.shape == x.grad.shape
        print(f"restatement {name},{mode} dlogits {LR.rel_err(d, x.grad):.3e} (of the largest |ref|: {LR.grad_err(d, x.grad):.3e})")
        assert LR.rel_err(d, x.grad) <= TIGHT, (mode, LR.rel_err(d, x.grad))


def test_the_table_reaches_what_it_names():
    """Every lattice kernel at both ends of its range, the tight and infeasible clips as such, and the special cases flagged."""
    S = {n: 2 * LR.CASES[n]["max_labels"] + 1 for n in LR.CASE_NAMES}
    assert [S[n] for n in LR.CASE_NAMES[:9]] == [63, 65, 127, 129, 255, 257, 511, 513, 1023]
    assert all(S[n] == 65 for n in LR.CASE_NAMES if n.endswith("_wide32"))
    for n in ("tight", "tight_wide32", "tight_L40"):
        c = LR.CASES[n]
        assert c["T"] == len(c["labels"][0]) + LR.repeats(c["labels"][0]) and LR.repeats(c["labels"][0]) >= 1
    for n in ("infeasible_beside_feasible", "infeasible_beside_feasible_wide32"):
        assert [LR.clip_state(LR.CASES[n], b) for b in (0, 1)] == ["infeasible", "ok"]
    assert [LR.clip_state(LR.CASES["empty_between_feasible"], b) for b in range(3)] == ["ok", "empty", "ok"]
    assert [LR.clip_state(LR.CASES["label_class_V_and_negative"], b) for b in range(3)] == ["infeasible", "ok", "infeasible"]
    special = [n for n in LR.CASE_NAMES if LR.make(n)["special"]]
    assert sorted(special) == sorted(["infeasible_beside_feasible", "infeasible_beside_feasible_wide32", "empty_between_feasible",
                                      "label_class_V_and_negative", "frames_all_ignored"])
    c = LR.make("logits_blank_spike_T40_V5_L6")
    assert float((c["x"][0, ::3, 1:5].amax(-1) - c["x"][0, ::3, 0]).max()) <= -88.0            # expf(m1 - m0) is 0 in float32
    assert len(LR.OFFSET_CASES) == 6


def test_the_cases_torch_does_not_define():
    # a clip without labels between two feasible ones: nll 0, no CTC gradient, the mean still over B = 3
    c = LR.make("empty_between_feasible")
    losses, nll, d = LR.losses_and_grad(c["x"], c["fl"], c["lab"], c["n_labels"], c["V"], 1.0, 0, 1)
    assert float(nll[1]) == 0.0 and not d[1].any() and d[0].any() and d[2].any() and not d[..., c["V"]].any()
    alone = []
    for b in (0, 2):        # each feasible clip alone: the same nll, and its rows are the batch's rows times B
        l1, n1, d1 = LR.losses_and_grad(c["x"][b: b + 1], c["fl"][b: b + 1], c["lab"][b: b + 1], c["n_labels"][b: b + 1], c["V"], 1.0, 0, 1)
        assert abs(float(n1[0]) - float(nll[b])) <= TIGHT * float(nll[b]) and LR.grad_err(d[b] * 3, d1[0]) <= TIGHT
        alone.append(float(l1[2]))
    assert abs(float(losses[2]) - sum(alone) / 3) <= TIGHT * float(losses[2])
    # no path: +inf, zero rows, the batch mate as if alone (its rows times B)
    for name, bad, good in (("infeasible_beside_feasible", [0], 1), ("label_class_V_and_negative", [0, 2], 1)):
        c = LR.make(name)
        losses, nll, d = LR.losses_and_grad(c["x"], c["fl"], c["lab"], c["n_labels"], c["V"], 1.0, 0, 1)
        assert float(losses[2]) == math.inf and all(float(nll[b]) == math.inf for b in bad) and math.isfinite(float(nll[good]))
        assert all(not d[b].any() for b in bad)
        _, n1, d1 = LR.losses_and_grad(c["x"][good: good + 1], c["fl"][good: good + 1], c["lab"][good: good + 1],
                                       c["n_labels"][good: good + 1], c["V"], 1.0, 0, 1)
        assert abs(float(n1[0]) - float(nll[good])) <= TIGHT * float(nll[good]) and LR.grad_err(d[good] * c["B"], d1[0]) <= TIGHT
    # one frame fewer than labels + repeats has no path, exactly that many has one
    c = LR.make("tight")
    assert math.isfinite(float(LR.losses_and_grad(c["x"], c["fl"], c["lab"], c["n_labels"], c["V"], 1.0, 0, 1)[1][0]))
    assert float(LR.losses_and_grad(c["x"][:, :-1], c["fl"][:, :-1], c["lab"], c["n_labels"], c["V"], 1.0, 0, 1)[1][0]) == math.inf
    # frame labels 0, V and V + 3 are the same as -100 for the word CE and as a label for the silence BCE
    c = LR.make("frames_0_and_V")
    V, fl = c["V"], c["fl"]
    assert int(((fl == 0) | (fl >= V)).sum()) == 3 * c["B"]
    losses, _, d = LR.losses_and_grad(c["x"], fl, c["lab"], c["n_labels"], V, 1.0, 1, 0)
    odd = (fl != -100) & ~((fl >= 1) & (fl < V))
    assert not d[..., :V][odd].any() and bool((d[..., V][odd] > 0).all())
    # no frame with a label: NaN, no word-CE gradient, the BCE gradient intact
    c = LR.make("frames_all_ignored")
    losses, _, d = LR.losses_and_grad(c["x"], c["fl"], c["lab"], c["n_labels"], c["V"], 1.0, 1, 0)
    assert math.isnan(float(losses[0])) and math.isfinite(float(losses[1])) and not d[..., : c["V"]].any()
    xs = c["x"][..., c["V"]].double()
    assert LR.grad_err(d[..., c["V"]], (torch.sigmoid(xs) - 1.0) / (c["B"] * c["T"])) <= TIGHT


@pytest.mark.parametrize("name", LR.OFFSET_CASES)
def test_the_float32_yardstick_does_not_fold_the_offset(name):
    """With +-1e4 on every word column, a folded normaliser (m + log s in one float) costs an ulp of 1e4 per frame: 5e-4.  e32 must stay at
    float32 round-off of the log-probabilities themselves."""
    (losses, nll, d), (l32, n32, d32) = LR.reference(name, "both")
    e_d, e_nll = LR.grad_err(d32, d), float((n32 - nll).abs().max())
    print(f"e32 {name} dlogits {e_d:.3e} nll {e_nll:.3e}")
    assert e_d <= 1e-6 and e_nll <= 1e-5
    assert LR.rel_err(l32, losses) <= 1e-6


def _args(**kw):
    """A valid call of la_multitask_loss on stand-in pointers (never launched: every test changes one argument into an invalid one)."""
    P = 4096                                      # non-null, 256-byte aligned, never dereferenced
    B, T, V, L = 2, 10, 6, 3
    a = dict(logits=P, batch_stride=T * (V + 1), row_stride=V + 1, batch=B, frames=T, vocab=V, frame_labels=P, ctc_labels=P, labels_stride=L,
             n_labels=P, max_labels=L, use_ce=1, use_ctc=1, scale=1.0, losses=P, dlogits=P, d_batch_stride=T * (V + 3), d_row_stride=V + 3,
             workspace=P, workspace_bytes=None, stream=0)
    a.update(kw)
    return a


def _call(L, a):
    need = ctypes.c_size_t(0)
    if a["workspace_bytes"] is None:
        assert L.la_multitask_loss_workspace_bytes(max(1, a["batch"]), max(1, a["frames"]), max(1, min(a["max_labels"], 511)), ctypes.byref(need)) == 0
        a["workspace_bytes"] = need.value
    return L.la_multitask_loss(*[a[k] for k in ("logits", "batch_stride", "row_stride", "batch", "frames", "vocab", "frame_labels", "ctc_labels",
                                                "labels_stride", "n_labels", "max_labels", "use_ce", "use_ctc", "scale", "losses", "dlogits",
                                                "d_batch_stride", "d_row_stride", "workspace", "workspace_bytes", "stream")])


def test_multitask_loss_rejects_bad_arguments_on_the_host():
    """Each call must come back LA_EINVAL from the host check, before any launch (the pointers are stand-ins)."""
    from lyricalignment_amd import _lib
    L = _lib.lib()
    E = _lib.LA_EINVAL
    need = ctypes.c_size_t(0)
    assert L.la_multitask_loss_workspace_bytes(2, 10, 3, ctypes.byref(need)) == 0 and need.value > 0 and need.value % 256 == 0
    bad = [(dict(logits=0), "null pointer"), (dict(losses=0), "null pointer"), (dict(workspace=0), "null pointer"),
           (dict(vocab=2, row_stride=7), "bad sizes"), (dict(batch=0), "bad sizes"), (dict(frames=0, batch_stride=0), "bad sizes"),
           (dict(row_stride=6, batch_stride=60), "dense rows"),                                   # row_stride < vocab + 1
           (dict(batch_stride=10 * 7 + 1), "dense rows"),                                         # batch_stride != frames * row_stride
           (dict(frame_labels=0), "CE requested without frame labels"),
           (dict(ctc_labels=0), "CTC requested without labels"), (dict(n_labels=0), "CTC requested without labels"),
           (dict(labels_stride=2), "CTC requested without labels"),                               # labels_stride < max_labels
           (dict(max_labels=0, labels_stride=0), "CTC requested without labels"),
           (dict(d_row_stride=6, d_batch_stride=60), "dlogits layout"), (dict(d_batch_stride=10 * 9 + 1), "dlogits layout"),
           (dict(max_labels=512, labels_stride=512), "more than 511 labels"),
           (dict(workspace_bytes=need.value - 1), "workspace too small or misaligned"),
           (dict(workspace=4096 + 128), "workspace too small or misaligned")]
    for change, message in bad:
        assert _call(L, _args(**change)) == E, change
        assert message in _lib.last_error(), (change, _lib.last_error())
    # the same checks hold for a losses-only call and for either term alone
    assert _call(L, _args(dlogits=0, d_batch_stride=0, d_row_stride=0, workspace_bytes=need.value - 1)) == E
    assert _call(L, _args(use_ctc=0, frame_labels=0)) == E and _call(L, _args(use_ce=0, ctc_labels=0)) == E
    # the workspace query
    for args in ((0, 10, 3), (2, 0, 3), (2, 10, 0), (-1, 10, 3)):
        assert L.la_multitask_loss_workspace_bytes(*args, ctypes.byref(need)) == E, args
        assert "multitask_loss_workspace_bytes" in _lib.last_error()
    assert L.la_multitask_loss_workspace_bytes(2, 10, 3, None) == E


def test_workspace_query_counts_two_floats_per_row_and_normaliser():
    """The query is what callers size the buffer by: accumulators (256 bytes), maximum and log-sum of both normalisers of every row,
    nll per clip, and the alpha rows of 2 max_labels + 1 states padded to a multiple of 4 doubles, every part rounded up to 256 bytes."""
    from lyricalignment_amd import _lib
    L = _lib.lib()
    up = lambda n: (n + 255) // 256 * 256
    need = ctypes.c_size_t(0)
    for B, T, Lmax in ((1, 1, 1), (2, 10, 3), (3, 33, 32), (2, 530, 511)):
        assert L.la_multitask_loss_workspace_bytes(B, T, Lmax, ctypes.byref(need)) == 0
        s_pad = (2 * Lmax + 1 + 3) // 4 * 4
        assert need.value == 256 + 2 * up(B * T * 8) + up(B * 4) + up(B * T * s_pad * 8), (B, T, Lmax)
