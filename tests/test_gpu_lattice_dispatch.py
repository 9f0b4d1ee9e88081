"""Which lattice entry points a call reaches: utils.alignment.perform_viterbi* and AlignModel.align against what this file composes
from the public ops.* calls, for every combination of optional spans, frame windows and confidence keyword.  The dispatch is restated
ONCE below, as data (DISPATCH); each combination either raises the ValueError it is listed with or equals the composition value for
value (== on Python floats, torch.equal on device tensors).  The kernels themselves are pinned by the suites of each face; this file
pins the host path that chooses among them, and the row pitch of span_skip_prob under a skip_from wider than Lmax + 1.
"""
import pytest
import torch

import windows_reference as wr

pytestmark = pytest.mark.gpu

HOP = 0.02
PENALTY = 2.0
BOUNDARY = 2

# (confidence, spans given, windows given) -> (DP entry, posteriors entry, where log_z_free comes from) or the ValueError's text.
# An all-empty keyword counts as not given.  Where the DP is viterbi_batch, AlignModel.align takes the fused head's own (the same
# kernel on the same emissions) except under return_anchored_confidence; alignment_posteriors_spans without spans gets an all -1
# skip_from; log_z_free "log_z" is the posteriors' own log_z (no windows), otherwise [3] of one more call of the entry named.
NO_WINDOW_POSTERIORS = "no posteriors on the windowed lattice"
DISPATCH = {
    (None, False, False): ("viterbi_batch", None, None),
    (None, True, False): ("viterbi_spans_batch", None, None),
    (None, False, True): ("viterbi_windows_batch", None, None),
    (None, True, True): ("viterbi_windows_batch", None, None),
    ("plain", False, False): ("viterbi_batch", "alignment_posteriors", None),
    ("span", False, False): ("viterbi_batch", "alignment_posteriors_spans", None),
    ("span", True, False): ("viterbi_spans_batch", "alignment_posteriors_spans", None),
    ("anchored", False, False): ("viterbi_batch", "alignment_posteriors_spans", "log_z"),
    ("anchored", True, False): ("viterbi_spans_batch", "alignment_posteriors_spans", "log_z"),
    ("anchored", False, True): ("viterbi_windows_batch", "alignment_posteriors_windows", "alignment_posteriors"),
    ("anchored", True, True): ("viterbi_windows_batch", "alignment_posteriors_windows", "alignment_posteriors_spans"),
}
FIELDS = ("onset", "offset", "score", "status", "occupancy", "onset_prob", "offset_prob", "log_z", "present_prob", "span_skip_prob",
          "log_z_free")


def _compose(key, em, lab, n_lab, nf, skip, win, head_dp=None):
    """DISPATCH[key] carried out with the public ops calls -> {field: device tensor}; skip / win are device tensors or None."""
    from lyricalignment_amd import ops
    dp_name, post_name, free_name = DISPATCH[key]
    if dp_name == "viterbi_batch":
        dp = head_dp if head_dp is not None else ops.viterbi_batch(em, lab, n_lab, nf)
    elif dp_name == "viterbi_spans_batch":
        dp = ops.viterbi_spans_batch(em, lab, n_lab, nf, skip, PENALTY)
    else:
        dp = ops.viterbi_windows_batch(em, lab, n_lab, nf, win[0], win[1], skip, PENALTY)
    out = dict(zip(FIELDS, dp))
    on, off = dp[0], dp[1]
    if post_name == "alignment_posteriors":
        post = ops.alignment_posteriors(em, lab, n_lab, nf, on, off, BOUNDARY)
    elif post_name == "alignment_posteriors_spans":
        rows = skip if skip is not None else torch.full((em.shape[0], lab.shape[1] + 1), -1, dtype=torch.int32, device=em.device)
        post = ops.alignment_posteriors_spans(em, lab, n_lab, nf, on, off, rows, PENALTY, BOUNDARY)
    elif post_name == "alignment_posteriors_windows":
        post = ops.alignment_posteriors_windows(em, lab, n_lab, nf, on, off, win[0], win[1], skip, PENALTY, BOUNDARY)
    else:
        return out
    out.update(zip(FIELDS[4:8], post[:4]))
    if len(post) > 5:
        out.update(present_prob=post[5], span_skip_prob=post[6])
    if free_name == "log_z":
        out["log_z_free"] = out["log_z"]
    elif free_name == "alignment_posteriors":
        out["log_z_free"] = ops.alignment_posteriors(em, lab, n_lab, nf, on, off, BOUNDARY)[3]
    elif free_name == "alignment_posteriors_spans":
        out["log_z_free"] = ops.alignment_posteriors_spans(em, lab, n_lab, nf, on, off, skip, PENALTY, BOUNDARY)[3]
    return out


def _formatted(r, lists, spans):
    """The composition as the public functions hand it over: seconds, or (seconds, scores) when posteriors were composed."""
    assert r["status"].tolist() == [0] * len(lists)
    on, off = r["onset"].cpu().numpy(), r["offset"].cpu().numpy()
    seconds = [[None if on[b, n] < 0 else [float(int(on[b, n])) * HOP, float(int(off[b, n])) * HOP] for n in range(len(labs))]
               for b, labs in enumerate(lists)]
    if "occupancy" not in r:
        return seconds
    host = {k: v.cpu().numpy() for k, v in r.items()}
    scores = []
    for b, labs in enumerate(lists):
        L = len(labs)
        d = {"occupancy": [float(v) for v in host["occupancy"][b, :L]], "onset_prob": [float(v) for v in host["onset_prob"][b, :L]],
             "offset_prob": [float(v) for v in host["offset_prob"][b, :L]], "path_log_posterior": float(host["score"][b] - host["log_z"][b])}
        if "present_prob" in r and spans is not None:
            d["sung_prob"] = [float(v) for v in host["present_prob"][b, :L]]
            d["span_skip_prob"] = [float(host["span_skip_prob"][b, n]) for _, n in spans[b]]
        if "log_z_free" in r:
            d["window_log_prob"] = float(host["log_z"][b] - host["log_z_free"][b])
        scores.append(d)
    return seconds, scores


# ------------------------------------------------------------------------------------------------ 1. perform_viterbi*
B, T, V = 2, 24, 12
LABELS = [[3, 5, 3, 7, 2], [4, 6, 9]]
N_FRAMES = [24, 17]
SPANS = [[(1, 2), (3, 5)], []]            # (1, 2): labels[2] == labels[0], the equal-neighbour case of the jump from J - 1
KINDS = {"": None, "_scored": "scored", "_anchored_scored": "anchored"}


@pytest.fixture(scope="module")
def matrix():
    """Seeded logits, per variant the emissions, and a char_windows / onset_anchors pair laid around the unconstrained path."""
    from lyricalignment_amd import _lib, ops
    from lyricalignment_amd.utils import alignment as ua
    logits = (torch.randn((B, T, V), generator=torch.Generator().manual_seed(7)) * 3).cuda()
    labels = torch.full((B, 5), -100, dtype=torch.long)
    for b, l in enumerate(LABELS):
        labels[b, : len(l)] = torch.tensor(l)
    lab, n_lab, lists = ua._labels_to_device(labels, B, logits.device)
    assert lists == LABELS
    nf = torch.tensor(N_FRAMES, dtype=torch.int32).cuda()
    skip = ua._skip_from_of_spans(SPANS, lists)
    out = dict(logits=logits, labels=labels, lab=lab, n_lab=n_lab, nf=nf, lists=lists, skip=skip.cuda())
    for ctc, variant in ((False, _lib.LA_VARIANT_PLAIN), (True, _lib.LA_VARIANT_CTC)):
        em = ops.emissions_from_logits(logits, lab, n_lab, variant)
        on, off, _, status = ops.viterbi_batch(em, lab, n_lab, nf)
        assert status.tolist() == [0, 0]
        cw = [[(2, (int(on[0, 2]) - 1) * HOP, (int(off[0, 2]) + 1) * HOP)], []]
        anchors = [[], [(1, int(on[1, 1]) * HOP, HOP)]]
        lo, hi = ua._windows_of(cw, anchors, lists, N_FRAMES, HOP)
        assert (lo[:, :7] > 0).any() and (hi[0, :11] < 24).any() and (hi[1, :7] < 17).any()          # the windows do constrain
        em_host = em.cpu().numpy()
        for rows in (None, skip):                                                                     # a path exists: on the host reference
            for b, l in enumerate(LABELS):
                S = 2 * len(l) + 1
                ref = wr.viterbi_windows(em_host[b, : N_FRAMES[b]], l, lo[b, :S].tolist(), hi[b, :S].tolist(),
                                         None if rows is None else rows[b, : len(l) + 1].tolist(), PENALTY)
                assert ref[3] == wr.LA_OK, (ctc, b, rows is None)
        out[ctc] = dict(em=em, cw=cw, anchors=anchors, win=(lo.cuda(), hi.cuda()))
    return out


@pytest.mark.parametrize("ctc", [False, True], ids=["plain_variant", "ctc"])
@pytest.mark.parametrize("suffix", list(KINDS))
def test_perform_viterbi_keyword_matrix(matrix, suffix, ctc):
    from lyricalignment_amd.utils import alignment as ua
    m, v = matrix, matrix[ctc]
    fn = getattr(ua, "perform_viterbi" + ("_ctc" if ctc else "") + suffix)
    kind = KINDS[suffix]
    n_checked = 0
    for spans in (None, [[], []], SPANS):
        for cw, anchors in ((None, None), ([[], []], [[], []]), (v["cw"], v["anchors"])):
            has_spans, has_win = spans is SPANS, cw is v["cw"]
            what = (suffix, ctc, spans, cw is not None, has_win)
            kw = dict(n_frames=N_FRAMES, optional_spans=spans, skip_penalty=PENALTY, char_windows=cw, onset_anchors=anchors)
            if kind is not None:
                kw["boundary_window"] = BOUNDARY
            if kind == "scored" and has_win:
                with pytest.raises(ValueError, match=NO_WINDOW_POSTERIORS):
                    fn(m["logits"], m["labels"], **kw)
                n_checked += 1
                continue
            conf = {None: None, "anchored": "anchored", "scored": "span" if has_spans else "plain"}[kind]
            r = _compose((conf, has_spans, has_win), v["em"], m["lab"], m["n_lab"], m["nf"], m["skip"] if has_spans else None,
                         v["win"] if has_win else None)
            # the scored functions name the spans only where one exists; the anchored ones always hold sung_prob / span_skip_prob
            want = _formatted(r, m["lists"], spans if has_spans else ([[], []] if kind == "anchored" else None))
            got = fn(m["logits"], m["labels"], **kw)
            assert got == want, what
            if kind is not None:
                keys = {"occupancy", "onset_prob", "offset_prob", "path_log_posterior"}
                keys |= {"sung_prob", "span_skip_prob"} if conf != "plain" else set()
                keys |= {"window_log_prob"} if kind == "anchored" else set()
                assert all(set(d) == keys for d in got[1]), what
                if kind == "anchored" and not has_win:
                    assert all(d["window_log_prob"] == 0.0 for d in got[1]), what
            n_checked += 1
    assert n_checked == 9


# ------------------------------------------------------------------------------------------------ 2. AlignModel.align
IDX = [1, 5]                                                 # clips of tests/test_gpu_ragged.py: 5 and 3 labels, 76 and 28 frames
ALIGN_SPANS = [[(1, 3), (3, 5)], [(0, 2)]]
FRAME_TUPLE = {None: 4, "plain": 8, "span": 10, "anchored": 11}
ERR_ANCHORED = "return_anchored_confidence does not go with"
ERR_WINDOWS = "do not go with return_confidence / return_span_confidence"
ERR_SPANS = "return_confidence is not defined with optional_spans"
ERRORS = (ERR_ANCHORED, ERR_WINDOWS, ERR_SPANS)


@pytest.fixture(scope="module")
def tiny():
    import test_gpu_ragged as tr
    from test_gpu_parity_full import _build
    model, _ = _build("tiny", torch.float32)
    return dict(model=model, audios=[tr._clip(i) for i in IDX], labels=tr._padded_labels(IDX), tr=tr)


def _expected_of_align(r_conf, r_span, r_anch, has_spans, has_win):
    """-> the confidence of DISPATCH's key, or the ValueError's text: the decision tree of align's keywords, in the order it raises."""
    if r_anch and (r_conf or r_span):
        return ERR_ANCHORED
    if r_anch:
        return "anchored"
    if has_win and (r_conf or r_span):
        return ERR_WINDOWS
    if has_spans and r_conf:
        return ERR_SPANS
    return "span" if r_span else "plain" if r_conf else None


@pytest.mark.parametrize("per_clip", [False, True])
def test_align_keyword_matrix(tiny, per_clip):
    import test_gpu_windows as tgw
    from lyricalignment_amd import _lib
    from lyricalignment_amd.module.align_model import N_CTX
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels, tr = tiny["model"], tiny["audios"], tiny["labels"], tiny["tr"]
    eng = model.engine()
    with torch.no_grad():
        # the emissions align() hands to the lattice: the head's, through the call align() makes
        if per_clip:
            feats, nb, Tmax, nf, counts = model._features_per_clip(audios)
            stride, kw_head = N_CTX, dict(n_frames=nf)
            assert counts == [tr.TS[i] for i in IDX]
        else:
            feats, nb, Tmax, stride = model._features(model._mel_of(audios).to(eng.device), True)
            nf, kw_head, counts = torch.full((nb,), Tmax, dtype=torch.int32, device=eng.device), {}, [Tmax] * nb
        lab, n_lab, lists = ua._labels_to_device(labels, nb, eng.device)
        *head_dp, em = eng.align_feats_checked(feats, nb, Tmax, stride, lab, n_lab, _lib.LA_VARIANT_CTC, want_emissions=True, **kw_head)
        fused_dp = eng.align_feats_checked(feats, nb, Tmax, stride, lab, n_lab, _lib.LA_VARIANT_CTC, **kw_head)     # the default path's call
        free = model.align(audios, labels, per_clip=per_clip, return_frames=True)
        assert len(free) == 4 and all(torch.equal(a, b) for a, b in zip(free, fused_dp))
        anchors, _ = tgw._anchors_off_the_free_result(free[0].tolist(), [len(l) for l in lists], counts)
        lo, hi = ua._windows_of(None, anchors, lists, counts, HOP)
        win = (lo.to(eng.device), hi.to(eng.device))
        skip = ua._skip_from_of_spans(ALIGN_SPANS, lists).to(eng.device)
        seen = set()
        for flags in range(8):
            r_conf, r_span, r_anch = bool(flags & 1), bool(flags & 2), bool(flags & 4)
            for has_spans in (False, True):
                for has_win in (False, True):
                    conf = _expected_of_align(r_conf, r_span, r_anch, has_spans, has_win)
                    kw = dict(per_clip=per_clip, return_confidence=r_conf, return_span_confidence=r_span, return_anchored_confidence=r_anch,
                              boundary_window=BOUNDARY, optional_spans=ALIGN_SPANS if has_spans else None, skip_penalty=PENALTY,
                              onset_anchors=anchors if has_win else None)
                    what = (per_clip, r_conf, r_span, r_anch, has_spans, has_win)
                    seen.add(conf)
                    if conf in ERRORS:
                        for return_frames in (False, True):
                            with pytest.raises(ValueError, match=conf):
                                model.align(audios, labels, return_frames=return_frames, **kw)
                        continue
                    # the plain lattice's DP is the fused head's, except under return_anchored_confidence (ops.viterbi_batch: the same bits)
                    r = _compose((conf, has_spans, has_win), em, lab, n_lab, nf, skip if has_spans else None, win if has_win else None,
                                 head_dp=None if conf == "anchored" else fused_dp if conf is None else tuple(head_dp))
                    frames = model.align(audios, labels, return_frames=True, **kw)
                    assert isinstance(frames, tuple) and len(frames) == FRAME_TUPLE[conf], what
                    for name, t in zip(FIELDS, frames):
                        assert t.is_cuda and t.dtype == r[name].dtype and t.shape == r[name].shape, (what, name)
                        assert t.cpu().numpy().tobytes() == r[name].cpu().numpy().tobytes(), (what, name)
                    spans = ALIGN_SPANS if has_spans else ([[]] * nb if conf in ("span", "anchored") else None)
                    assert model.align(audios, labels, **kw) == _formatted(r, lists, spans), what
        assert seen == {None, "plain", "span", "anchored", *ERRORS}


# ------------------------------------------------------------------------------------------------ 3. a skip_from wider than Lmax + 1
def test_wide_skip_from_keeps_span_skip_prob_inside_its_buffer():
    """skip_from as a [2, 4] slice of a [2, 8] tensor (row pitch 8; the kernel addresses span_skip_prob with the pitch it is told): the
    seven outputs of alignment_posteriors_spans and alignment_posteriors_windows (open windows) are those of a contiguous [2, 4]
    skip_from bit for bit, and span_skip_prob is [2, 4]."""
    from lyricalignment_amd import ops
    nb, nt, L = 2, 8, 3
    em = (-torch.rand((nb, nt, L + 1), generator=torch.Generator().manual_seed(3)) * 4).cuda()
    lab = torch.tensor([[2, 3, 2], [4, 5, 6]], dtype=torch.int32).cuda()
    n_lab = torch.full((nb,), L, dtype=torch.int32).cuda()
    nf = torch.full((nb,), nt, dtype=torch.int32).cuda()
    wide = torch.full((nb, 8), -1, dtype=torch.int32)
    wide[0, 2], wide[1, 3] = 0, 1
    wide = wide.cuda()[:, : L + 1]
    tight = wide.contiguous()
    assert wide.stride(0) == 8 and tight.stride(0) == L + 1 and wide.shape == tight.shape == (nb, L + 1)
    lo = torch.zeros((nb, 2 * L + 1), dtype=torch.int32).cuda()
    hi = torch.full((nb, 2 * L + 1), nt, dtype=torch.int32).cuda()
    on, off, _, status = ops.viterbi_spans_batch(em, lab, n_lab, nf, tight, 0.5)
    assert status.tolist() == [0, 0]
    for name, call in (("spans", lambda s: ops.alignment_posteriors_spans(em, lab, n_lab, nf, on, off, s, 0.5, BOUNDARY)),
                       ("windows", lambda s: ops.alignment_posteriors_windows(em, lab, n_lab, nf, on, off, lo, hi, s, 0.5, BOUNDARY))):
        want, got = call(tight), call(wide)
        torch.cuda.synchronize()
        assert len(want) == len(got) == 7
        assert got[6].shape == want[6].shape == (nb, L + 1), name
        for i, (w, g) in enumerate(zip(want, got)):
            assert w.shape == g.shape and w.cpu().numpy().tobytes() == g.cpu().numpy().tobytes(), (name, i)
        assert float(got[6].sum()) > 0.0, name                     # the spans carry mass: the comparison is not of zeros
