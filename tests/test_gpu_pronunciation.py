"""Pronunciation scores on the device (csrc/la_pronunciation.hip: la_segment_class_scores sums every candidate class over the segment the
DP gave a position, ranks the position's own class and names the top few) and the layers over it (ops.segment_class_scores, the
return_pronunciation / pronunciation_classes / pronunciation_top_k keywords of perform_viterbi(_ctc) and AlignModel.align, the sheet
functions of the harness and harness.suspect_characters).

Yardstick: pronunciation_reference (float64 numpy; an explicit sequential loop per segment, a stable sort on (-score, column)), and for
the lattice repeat_spans_reference.viterbi run on the emissions the device produced.

Bound, derived and never measured: the segment sums are sequential float64 additions of the same float32 inputs in the same order, and
the selection compares those sums exactly: every output of the kernel is bit-equal to the restatement.  The public dicts divide two such
numbers in float64 on both sides: equal."""
import functools

import numpy as np
import pytest
import torch

import pronunciation_reference as pr
import readings_reference as rdr
import repeat_spans_reference as rr
from test_gpu_repeat_spans import _planted_logits

pytestmark = pytest.mark.gpu

HOP = 0.02
SENT_F, SENT_I = -77.25, -7777                    # what the outputs hold before a call: no sum, column, rank or count of a case equals them
FILL = {"seg_score": SENT_F, "top_col": SENT_I, "top_score": SENT_F, "own_score": SENT_F, "own_rank": SENT_I, "n_seg_frames": SENT_I}
NAMES = ("top_col", "top_score", "own_score", "own_rank", "n_seg_frames", "seg_score")


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ------------------------------------------------------------------------------------------------ 1. the kernel against the restatement
T_MAX = 53
# hand-made disjoint segments of the 7-label clip: one frame; an ordinary one; skipped; the longest (more than one load-ahead group and a
# tail); one frame again; skipped; an offset beyond max_frames (clamped).  The 1-label clip's segment ends at max_frames exactly.
SEGMENTS = [[(0, 1), (3, 10), (-1, -1), (10, 31), (31, 32), (-1, -1), (40, 60)], [(20, T_MAX)], []]


@functools.lru_cache(maxsize=None)
def kernel_case(C):
    """-> em [3, 53, C] float32, n_labels, onset / offset / own_col [3, 7]: random emissions, ragged label counts 7 / 1 / 0."""
    rs = np.random.RandomState(1000 + C)
    em = (-rs.rand(3, T_MAX, C) * 12.0).astype(np.float32)
    n_labels = [len(s) for s in SEGMENTS]
    Lmax = max(n_labels)
    onset = np.full((3, Lmax), -1, dtype=np.int32)
    offset = np.full((3, Lmax), -1, dtype=np.int32)
    own = rs.randint(0, C, size=(3, Lmax)).astype(np.int32)
    own[0, 4] = -1                                                    # a sung position without an own column
    for b, segs in enumerate(SEGMENTS):
        for n, (t, u) in enumerate(segs):
            onset[b, n], offset[b, n] = t, u
    return em, n_labels, onset, offset, own


@functools.lru_cache(maxsize=None)
def kernel_reference(C, top_k):
    em, n_labels, onset, offset, own = kernel_case(C)
    return pr.segment_class_scores(em, n_labels, onset, offset, own, top_k, fill=FILL)


def _window(em, pad=3):
    """em [B, T, C] -> a device view of it as an OFFSET COLUMN WINDOW of a wider matrix with an odd row stride behind a one-element offset
    (no row start is 16-byte aligned), NaN wherever the kernel must not read."""
    B, T, C = em.shape
    WS = (pad + C + 2) | 1
    flat = torch.full((B * T * WS + 1,), float("nan"), dtype=torch.float32)
    flat[1:].view(B, T, WS)[:, :, pad: pad + C] = torch.from_numpy(np.ascontiguousarray(em))
    win = flat.cuda()[1:].view(B, T, WS)[:, :, pad: pad + C]
    assert win.stride() == (T * WS, WS, 1) and (win.data_ptr() % 16 != 0 or (WS * 4) % 16 != 0)
    return win


def _sentinel_outputs(B, Lmax, C, top_k):
    """Outputs wider than what the entry writes, full of sentinels: -> (the whole buffers by name, the views to hand to ops)."""
    whole = {"top_col": torch.full((B, Lmax, top_k + 2), SENT_I, dtype=torch.int32).cuda(),
             "top_score": torch.full((B, Lmax, top_k + 2), SENT_F, dtype=torch.float64).cuda(),
             "own_score": torch.full((B, Lmax + 3), SENT_F, dtype=torch.float64).cuda(),
             "own_rank": torch.full((B, Lmax + 3), SENT_I, dtype=torch.int32).cuda(),
             "n_seg_frames": torch.full((B, Lmax + 3), SENT_I, dtype=torch.int32).cuda(),
             "seg_score": torch.full((B, Lmax, C + 1), SENT_F, dtype=torch.float64).cuda()}
    views = (whole["top_col"][:, :, :top_k], whole["top_score"][:, :, :top_k], whole["own_score"][:, :Lmax], whole["own_rank"][:, :Lmax],
             whole["n_seg_frames"][:, :Lmax], whole["seg_score"][:, :, :C])
    return whole, views


def _assert_whole(whole, ref, what):
    """Every buffer: the reference (with the sentinel where the entry writes nothing) inside, the sentinel in the padding."""
    for name, t in whole.items():
        got = t.cpu().numpy()
        want = np.full(got.shape, FILL[name], dtype=got.dtype)
        want[tuple(slice(0, s) for s in ref[name].shape)] = ref[name]
        assert _same_bits(got, want), (what, name, np.argwhere(got != want)[:5])


@pytest.mark.parametrize("top_k", [1, 5, 16])
@pytest.mark.parametrize("C", [1, 5, 255, 256, 257, 402, 700])
def test_every_output_is_bit_equal_and_nothing_else_is_written(C, top_k):
    from lyricalignment_amd import ops
    em, n_labels, onset, offset, own = kernel_case(C)
    ref = kernel_reference(C, top_k)
    if top_k > C:                                                      # the case the issue names: trailing -1 / -inf
        assert (ref["top_col"][0, 0, C:] == -1).all() and np.isneginf(ref["top_score"][0, 0, C:]).all()
    assert ref["n_seg_frames"][0].tolist() == [1, 7, 0, 21, 1, 0, 13] and ref["n_seg_frames"][1, 0] == T_MAX - 20
    assert ref["own_rank"][0, 4] == -1 and ref["own_score"][0, 4] == 0.0 and ref["top_col"][0, 4, 0] >= 0
    whole, views = _sentinel_outputs(3, 7, C, top_k)
    out = ops.segment_class_scores(_window(em), torch.tensor(n_labels, dtype=torch.int32).cuda(), torch.from_numpy(onset).cuda(),
                                   torch.from_numpy(offset).cuda(), torch.from_numpy(own).cuda(), top_k=top_k, want_scores=True, out=views)
    assert len(out) == 6 and all(a is b for a, b in zip(out, views))
    _assert_whole(whole, ref, (C, top_k))
    # without the optional output, into the wrapper's own tensors: the same bits on every position a clip has
    got = ops.segment_class_scores(_window(em, pad=0), torch.tensor(n_labels, dtype=torch.int32).cuda(), torch.from_numpy(onset).cuda(),
                                   torch.from_numpy(offset).cuda(), torch.from_numpy(own).cuda(), top_k=top_k)
    assert len(got) == 5
    for name, t in zip(NAMES, got):
        for b, L in enumerate(n_labels):
            assert _same_bits(t[b, :L].cpu().numpy(), ref[name][b, :L]), (name, b)


def test_ties_go_to_the_smaller_column_in_the_order_and_in_the_rank():
    from lyricalignment_amd import ops
    rs = np.random.RandomState(7)
    T, C = 20, 300
    em = (-6.0 - rs.rand(1, T, C) * 6.0).astype(np.float32)
    em[0, :, 260] = em[0, :, 3] = (-rs.rand(T)).astype(np.float32)     # two identical columns, the best of all, in different waves
    em[0, :, 70] = em[0, :, 3] - np.float32(0.5)
    onset, offset = np.array([[2, 9, 15]], dtype=np.int32), np.array([[9, 15, 20]], dtype=np.int32)
    own = np.array([[260, 3, 70]], dtype=np.int32)                     # ties with a smaller column; is that smaller column; third
    ref = pr.segment_class_scores(em, [3], onset, offset, own, 5)
    assert ref["own_rank"][0].tolist() == [1, 0, 2] and ref["top_col"][0, :, :3].tolist() == [[3, 260, 70]] * 3
    assert (ref["top_score"][0, :, 0] == ref["top_score"][0, :, 1]).all()
    for n in range(3):
        sums = ref["seg_score"][0, n]
        assert pr.rank_by_count(sums, int(own[0, n])) == ref["own_rank"][0, n]
    got = ops.segment_class_scores(torch.from_numpy(em).cuda(), torch.tensor([3], dtype=torch.int32).cuda(), torch.from_numpy(onset).cuda(),
                                   torch.from_numpy(offset).cuda(), torch.from_numpy(own).cuda(), top_k=5, want_scores=True)
    for name, t in zip(NAMES, got):
        assert _same_bits(t.cpu().numpy(), ref[name]), name


def test_minus_infinity_and_the_floor_are_ordinary_values():
    from lyricalignment_amd import ops
    rs = np.random.RandomState(8)
    T, C = 30, 40
    em = (-rs.rand(1, T, C) * 10.0).astype(np.float32)
    em[0, 3:6, 5] = -np.inf                                            # -inf over a part of position 0's segment
    em[0, 0:4, 7] = -1000.0                                            # the floor over a part of it
    em[0, 4:10, 8] = -1000.0                                           # ... and over all of position 1's part below
    em[0, 20:25, :] = -np.inf                                          # position 2: every candidate impossible
    onset, offset = np.array([[0, 10, 20, 25]], dtype=np.int32), np.array([[10, 20, 25, 30]], dtype=np.int32)
    own = np.array([[5, 8, 17, 0]], dtype=np.int32)
    ref = pr.segment_class_scores(em, [4], onset, offset, own, 16)
    assert ref["own_score"][0, 0] == -np.inf and ref["own_rank"][0, 0] == C - 1 and ref["top_col"][0, 0, :].tolist().count(5) == 0
    assert np.isneginf(ref["top_score"][0, 2]).all() and ref["top_col"][0, 2].tolist() == list(range(16)) and ref["own_rank"][0, 2] == 17
    assert -7000.0 < ref["seg_score"][0, 0, 7] < -4000.0
    got = ops.segment_class_scores(torch.from_numpy(em).cuda(), torch.tensor([4], dtype=torch.int32).cuda(), torch.from_numpy(onset).cuda(),
                                   torch.from_numpy(offset).cuda(), torch.from_numpy(own).cuda(), top_k=16, want_scores=True)
    for name, t in zip(NAMES, got):
        assert _same_bits(t.cpu().numpy(), ref[name]), name


@pytest.mark.parametrize("shape", ["one_segment_of_3000_frames", "600_positions"])
def test_long_segments_and_whole_songs_are_bit_equal(shape):
    from lyricalignment_amd import ops
    rs = np.random.RandomState(9)
    C = 402
    if shape == "one_segment_of_3000_frames":
        T, L = 3000, 1
        onset, offset = np.array([[0]], dtype=np.int32), np.array([[T]], dtype=np.int32)
    else:
        T, L = 1500, 600
        cuts = np.sort(rs.choice(np.arange(1, T), size=2 * L - 1, replace=False))          # character, silence, character, ...
        bounds = np.concatenate([[0], cuts, [T]])
        onset, offset = bounds[0:2 * L:2][None].astype(np.int32), bounds[1:2 * L:2][None].astype(np.int32)
        onset[0, 100:110] = offset[0, 100:110] = -1                                         # a skipped line
    em = (-rs.rand(1, T, C) * 12.0).astype(np.float32)
    own = rs.randint(0, C, size=(1, L)).astype(np.int32)
    ref = pr.segment_class_scores(em, [L], onset, offset, own, 5)
    got = ops.segment_class_scores(_window(em), torch.tensor([L], dtype=torch.int32).cuda(), torch.from_numpy(onset).cuda(),
                                   torch.from_numpy(offset).cuda(), torch.from_numpy(own).cuda(), top_k=5, want_scores=True)
    for name, t in zip(NAMES, got):
        assert _same_bits(t.cpu().numpy(), ref[name]), name


def test_a_clip_has_the_same_bits_alone_in_a_batch_and_across_calls():
    from lyricalignment_amd import ops
    em, n_labels, onset, offset, own = kernel_case(402)

    def run(sel):
        return ops.segment_class_scores(torch.from_numpy(np.ascontiguousarray(em[sel])).cuda(),
                                        torch.tensor([n_labels[b] for b in sel], dtype=torch.int32).cuda(),
                                        torch.from_numpy(onset[sel]).cuda(), torch.from_numpy(offset[sel]).cuda(),
                                        torch.from_numpy(own[sel]).cuda(), top_k=5, want_scores=True)

    batch, again = run([0, 1, 2]), run([0, 1, 2])
    for b in (0, 1):
        alone = run([b])
        L = n_labels[b]
        for name, x, y, z in zip(NAMES, batch, again, alone):
            assert _same_bits(x[b, :L].cpu().numpy(), z[0, :L].cpu().numpy()), (name, b)
            assert _same_bits(x[b, :L].cpu().numpy(), y[b, :L].cpu().numpy()), (name, b)


def test_argument_errors_return_their_codes_and_leave_the_outputs_alone():
    from lyricalignment_amd import _lib, ops
    em, n_labels, onset, offset, own = kernel_case(5)
    B, T, C, Lmax, K = 3, T_MAX, 5, 7, 5
    emd = torch.from_numpy(em).cuda()
    nl, on, off, oc = (torch.from_numpy(np.asarray(a, dtype=np.int32)).cuda() for a in (n_labels, onset, offset, own))
    whole, v = _sentinel_outputs(B, Lmax, C, K)
    P = _lib.ptr
    wide = torch.full((2, B, Lmax + 3), -1, dtype=torch.int32).cuda()          # onset / offset share the row pitch of the [B, Lmax] outputs
    wide[0, :, :Lmax], wide[1, :, :Lmax] = on, off
    on, off = wide[0], wide[1]
    good = dict(em_c=P(emd), ebs=T * C, ers=C, n_labels=P(nl), onset=P(on), offset=P(off), out_stride=Lmax + 3, own_col=P(oc), own_stride=Lmax,
                batch=B, T=T, Lmax=Lmax, C=C, top_k=K, seg=P(v[5]), sbs=Lmax * (C + 1), srs=C + 1, top_col=P(v[0]), top_score=P(v[1]),
                top_stride=K + 2, own_score=P(v[2]), own_rank=P(v[3]), n_seg=P(v[4]))

    def call(**kw):
        a = {**good, **kw}
        return _lib.lib().la_segment_class_scores(*(a[k] for k in good), _lib.stream_ptr())

    cases = [(dict(**{k: 0}), _lib.LA_EINVAL, "null") for k in ("em_c", "n_labels", "onset", "offset", "own_col", "top_col", "top_score",
                                                              "own_score", "own_rank", "n_seg")]
    cases += [(dict(**{k: bad}), _lib.LA_EINVAL, "sizes") for k in ("batch", "T", "Lmax", "C", "top_k") for bad in (0, -1)]
    cases += [(dict(C=4096, ers=1), _lib.LA_EUNSUPPORTED, "4095"), (dict(Lmax=4096, out_stride=1), _lib.LA_EUNSUPPORTED, "4095"),
              (dict(top_k=17, top_stride=1), _lib.LA_EUNSUPPORTED, "16")]
    cases += [(kw, _lib.LA_EINVAL, "strides") for kw in (dict(ers=C - 1), dict(ebs=(T - 1) * C + C - 1), dict(out_stride=Lmax - 1),
                                                         dict(own_stride=Lmax - 1), dict(top_stride=K - 1), dict(srs=C - 1),
                                                         dict(sbs=(Lmax - 1) * (C + 1) + C - 1))]
    for kw, rc, what in cases:
        assert call(**kw) == rc, kw
        assert what in _lib.last_error() and "segment_class_scores" in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    for name, t in whole.items():                                      # nothing was enqueued: every sentinel is intact
        assert (t == FILL[name]).all(), name
    assert call() == _lib.LA_OK and call(seg=0, sbs=0, srs=0) == _lib.LA_OK          # the good call, with and without the optional output
    # the wrapper's own refusals
    on, off = on[:, :Lmax], off[:, :Lmax]
    with pytest.raises(NotImplementedError):
        ops.segment_class_scores(emd, nl, on, off, oc, top_k=17)
    with pytest.raises(ValueError):
        ops.segment_class_scores(emd, nl, on, off, oc, top_k=0)
    with pytest.raises(ValueError):
        ops.segment_class_scores(emd, nl, on[:, :6], off, oc)


# ------------------------------------------------------------------------------------------------ 2. the route
class _Spy:
    """ops.segment_class_scores with its arguments and results kept: the emissions the device produced are the reference's input."""

    def __init__(self, monkeypatch):
        from lyricalignment_amd import ops
        self.calls, self.inner = [], ops.segment_class_scores
        monkeypatch.setattr(ops, "segment_class_scores", self)

    def __call__(self, em_c, n_labels, onset, offset, own_col, top_k=5, want_scores=False, out=None):
        res = self.inner(em_c, n_labels, onset, offset, own_col, top_k, want_scores, out)
        self.calls.append(dict(em_c=em_c, n_labels=n_labels, onset=onset, offset=offset, own_col=own_col, top_k=top_k, res=res))
        return res

    def expected(self, classes):
        """The public list the last call must have led to: the restatement on what the entry was given."""
        c = self.calls[-1]
        em_c, nl, on, off, own = (c[k].cpu().numpy() for k in ("em_c", "n_labels", "onset", "offset", "own_col"))
        ref = pr.segment_class_scores(em_c, nl, on, off, own, c["top_k"])
        for name, t in zip(NAMES, c["res"]):
            for b, L in enumerate(nl):
                assert _same_bits(t[b, :L].cpu().numpy(), ref[name][b, :L]), (name, b)
        return [pr.pronunciation_dicts(ref, b, [classes[j] if j >= 0 else None for j in own[b, :L]], classes) for b, L in enumerate(nl)]


def _frames(seconds):
    return [None if s is None else (round(s[0] / HOP), round(s[1] / HOP)) for s in seconds]


@pytest.mark.parametrize("ctc", [True, False])
def test_candidate_columns_do_not_depend_on_the_list_they_sit_in(monkeypatch, ctc):
    from lyricalignment_amd import _lib, ops
    from lyricalignment_amd.utils import alignment as ua
    rs = np.random.RandomState(21)
    B, T, V = 2, 60, 46                                                # classes 1 .. 46: column 0 in front, the silence logit behind (CTC)
    pred = torch.from_numpy((rs.randn(B, T, V + (2 if ctc else 1)) * 3.0).astype(np.float32)).cuda()
    labels = torch.tensor([[5, 9, 5, 30, 46, 2, 41], [44, 3, 3, -100, -100, -100, -100]])
    f = ua.perform_viterbi_ctc if ctc else ua.perform_viterbi
    spy = _Spy(monkeypatch)
    plain = f(pred, labels)
    assert not spy.calls                                               # off: the call as it was
    seconds, pron = f(pred, labels, return_pronunciation=True, pronunciation_classes=40, pronunciation_top_k=3)
    assert seconds == plain                                            # the lattice read the same emissions
    classes = pr.candidate_classes(40, [[5, 9, 5, 30, 46, 2, 41], [44, 3, 3]])
    assert classes == list(range(1, 41)) + [41, 44, 46]
    em_c = spy.calls[-1]["em_c"]
    assert em_c.shape == (B, T, len(classes)) and em_c.stride(1) == 1 + 7 + len(classes)            # a window, not a copy
    as_labels = torch.tensor([classes] * B, dtype=torch.int32).cuda()
    alone = ops.emissions_from_logits(pred, as_labels, torch.full((B,), len(classes), dtype=torch.int32).cuda(),
                                      _lib.LA_VARIANT_CTC if ctc else _lib.LA_VARIANT_PLAIN)[:, :, 1:]
    diff = (em_c - alone).abs().max().item()
    print(f"ctc={ctc}: candidate columns in the widened rows against the same classes as plain labels: max |difference| {diff!r}")
    assert _same_bits(em_c.cpu().numpy(), alone.cpu().numpy())
    assert pron == spy.expected(classes)
    for b, row in enumerate(pron):
        for n, d in enumerate(row):
            assert d["class"] == int(labels[b, n]) and d["frames"] == _frames(seconds[b])[n][1] - _frames(seconds[b])[n][0]
            assert d["gop"] <= 0.0 and (d["gop"] == 0.0) == (d["rank"] == 0) and len(d["top"]) == 3
            assert (d["rank"] == 0) == (d["top"][0][0] == d["class"])
    # an explicit class list, unsorted and with repeats: sorted, unique, the sheet's own unioned in
    _, pron2 = f(pred, labels, return_pronunciation=True, pronunciation_classes=[12, 7, 7, 46], pronunciation_top_k=16)
    classes2 = sorted({12, 7, 46} | {5, 9, 30, 2, 41, 44, 3})
    assert spy.calls[-1]["em_c"].shape[2] == len(classes2) and pron2 == spy.expected(classes2) and len(pron2[0][0]["top"]) == len(classes2)


def test_a_planted_wrong_character_is_the_one_the_harness_reports():
    from lyricalignment_amd.harness import PinyinClassLUT, _pronunciation_lines, suspect_characters
    from lyricalignment_amd.utils import alignment as ua
    labels = torch.tensor([[4, 3, 9, 6, 2]])                           # the sheet says 9 at position 2 where the audio sings q = 7
    sung = [4, 3, 7, 6, 2]
    lg = _planted_logits(sung, 5 * (2 * len(sung) + 1), 12, 5).cuda()
    seconds, pron = ua.perform_viterbi_ctc(lg, labels, return_pronunciation=True, pronunciation_classes=10)
    assert seconds == ua.perform_viterbi_ctc(lg, labels)
    assert [d["rank"] == 0 for d in pron[0]] == [True, True, False, True, True]
    assert pron[0][2]["rank"] > 0 and pron[0][2]["top"][0][0] == 7 and pron[0][2]["gop"] < 0.0 and pron[0][2]["class"] == 9
    assert all(d["gop"] == 0.0 and d["top"][0][0] == d["class"] for n, d in enumerate(pron[0]) if n != 2)
    syllables = ["sil", "a", "bo", "ci", "de", "e", "fo", "ge", "he", "yi", "ji"]
    lut = PinyinClassLUT(syllables, {s: i for i, s in enumerate(syllables)})
    lines = ["一二", "三四五"]
    result = _pronunciation_lines(pron[0], lines, lut)
    assert [len(line) for line in result] == [2, 3] and result[1][0]["char"] == "三" and result[1][0]["syllable"] == "yi"
    assert suspect_characters(result) == [(1, 0, "ge", pron[0][2]["gop"])]
    assert suspect_characters(result, max_rank=len(syllables)) == []
    assert suspect_characters(result, max_rank=len(syllables), min_gop=pron[0][2]["gop"] / 2) == [(1, 0, "ge", pron[0][2]["gop"])]


def _restated(pred, labels_row, classes, variant, top_k, skip=None, pen=0.0, rf=None, rpen=0.0):
    """One clip of materialised logits -> (frames per position, the public pronunciation list) by the float64 restatements, on the
    emissions the device's prep gives for the widened rows."""
    from lyricalignment_amd import ops
    L = len(labels_row)
    lab_w = torch.tensor([list(labels_row) + classes], dtype=torch.int32).cuda()
    em_w = ops.emissions_from_logits(pred, lab_w, torch.tensor([L + len(classes)], dtype=torch.int32).cuda(), variant)[0].cpu().numpy()
    res = rr.viterbi(em_w[:, : L + 1], labels_row, skip, pen, rf, rpen, rows=True)
    assert res[3] == rr.LA_OK
    own = [[classes.index(c) for c in labels_row]]
    ref = pr.segment_class_scores(em_w[None, :, L + 1:], [L], [res[0]], [res[1]], own, top_k)
    return [None if t < 0 else (t, u) for t, u in zip(res[0], res[1])], pr.pronunciation_dicts(ref, 0, labels_row, classes)


def test_with_optional_spans_a_skipped_line_gives_none():
    from lyricalignment_amd import _lib
    from lyricalignment_amd.utils import alignment as ua
    labels = [4, 3, 9, 6]
    lg = _planted_logits([4, 3, 6], 5 * 7, 12, 5).cuda()               # the line "9" is not sung
    seconds, pron = ua.perform_viterbi_ctc(lg, torch.tensor([labels]), optional_spans=[[(2, 3)]], skip_penalty=0.25, return_pronunciation=True,
                                           pronunciation_classes=10)
    classes = pr.candidate_classes(10, [labels])
    frames, want = _restated(lg, labels, classes, _lib.LA_VARIANT_CTC, 5, skip=[-1, -1, -1, 2, -1], pen=0.25)
    assert seconds[0][2] is None and pron[0][2] is None and frames[2] is None
    assert _frames(seconds[0]) == frames and pron[0] == want and all(d["rank"] == 0 for d in pron[0] if d is not None)


def test_with_repeat_spans_the_first_visit_is_scored():
    from lyricalignment_amd import _lib
    from lyricalignment_amd.utils import alignment as ua
    labels = [3, 5, 7, 2, 9, 4]                                        # lines (3 5) (7 2) (9 4); the audio sings A B B C
    lg = _planted_logits([3, 5, 7, 2, 7, 2, 9, 4], 5 * 17, 12, 5).cuda()
    seconds, segments, pron = ua.perform_viterbi_ctc(lg, torch.tensor([labels]), repeat_spans=[[(2, 4)]], repeat_penalty=1.0,
                                                     return_segments=True, return_pronunciation=True, pronunciation_classes=10)
    classes = pr.candidate_classes(10, [labels])
    frames, want = _restated(lg, labels, classes, _lib.LA_VARIANT_CTC, 5, rf=[-1, -1, 4, -1, -1, -1], rpen=1.0)
    assert [n for n, _, _ in segments[0]] == [0, 1, 2, 3, 2, 3, 4, 5]
    assert _frames(seconds[0]) == frames == [(5 + 10 * i, 10 + 10 * i) for i in (0, 1, 2, 3, 6, 7)] and pron[0] == want
    assert [d["frames"] for d in pron[0]] == [5] * 6


def test_with_alternatives_the_own_class_is_the_reading_that_was_picked(monkeypatch):
    from lyricalignment_amd.utils import alignment as ua
    labels = torch.tensor([[4, 3, 9, 6]])                              # the sheet says 3 where the audio sings its other reading 7
    lg = _planted_logits([4, 7, 9, 6], 5 * 9, 12, 5).cuda()
    spy = _Spy(monkeypatch)
    seconds, readings, pron = ua.perform_viterbi_ctc(lg, labels, alternatives=[[(1, [7]), (2, [5])]], return_readings=True,
                                                     return_pronunciation=True, pronunciation_classes=[1, 2, 8])
    classes = [1, 2, 3, 4, 5, 6, 7, 8, 9]                              # every reading's class is a candidate
    assert (seconds, readings) == ua.perform_viterbi_ctc(lg, labels, alternatives=[[(1, [7]), (2, [5])]], return_readings=True)
    assert [r[0] for r in readings[0]] == [4, 7, 9, 6]
    assert spy.calls[-1]["own_col"][0].tolist() == [classes.index(c) for c in (4, 7, 9, 6)]
    assert pron == spy.expected(classes) and [d["class"] for d in pron[0]] == [4, 7, 9, 6] and all(d["rank"] == 0 for d in pron[0])
    assert spy.calls[-1]["em_c"].stride(1) == 1 + 6 + len(classes)      # behind the six expanded columns
    # without return_readings the readings are still picked for the own class, and not returned
    seconds2, pron2 = ua.perform_viterbi_ctc(lg, labels, alternatives=[[(1, [7]), (2, [5])]], return_pronunciation=True,
                                             pronunciation_classes=[1, 2, 8])
    assert seconds2 == seconds and pron2 == pron


def test_a_600_label_sheet(monkeypatch):
    from lyricalignment_amd import _lib
    from lyricalignment_amd.utils import alignment as ua
    rs = np.random.RandomState(33)
    T, L, V = 700, 600, 60
    labels = [int(v) for v in rs.randint(1, V + 1, size=L)]
    pred = torch.from_numpy((rs.randn(1, T, V + 2) * 2.0).astype(np.float32)).cuda()          # column 0, V classes, the silence logit
    seconds, pron = ua.perform_viterbi_ctc(pred, torch.tensor([labels]), return_pronunciation=True, pronunciation_classes=V, pronunciation_top_k=2)
    frames, want = _restated(pred, labels, list(range(1, V + 1)), _lib.LA_VARIANT_CTC, 2)
    assert seconds == ua.perform_viterbi_ctc(pred, torch.tensor([labels]))
    assert _frames(seconds[0]) == frames and pron[0] == want
    assert any(d["rank"] > 0 for d in pron[0]) and any(d["rank"] == 0 for d in pron[0])


# ------------------------------------------------------------------------------------------------ 3. the model
@pytest.fixture(scope="module")
def tiny():
    import test_gpu_ragged as tr
    from test_gpu_parity_full import _build
    model, _ = _build("tiny", torch.float32)
    idx = [0, 1, 3, 5]                                           # clips of tests/test_gpu_ragged.py: 11, 5, 8, 3 labels
    return dict(model=model, audios=[tr._clip(i) for i in idx], labels=tr._padded_labels(idx), tr=tr, idx=idx)


@pytest.mark.parametrize("use_ctc", [True, False])
def test_align_with_pronunciation_equals_the_restatement_on_the_heads_emissions(tiny, monkeypatch, use_ctc):
    model, audios, labels = tiny["model"], tiny["audios"], tiny["labels"]
    lists = [[int(v) for v in row if int(v) != -100] for row in labels]
    classes = pr.candidate_classes(40, lists)
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        plain = model.align(audios, labels, use_ctc=use_ctc)
        assert not spy.calls
        seconds, pron = model.align(audios, labels, use_ctc=use_ctc, return_pronunciation=True, pronunciation_classes=40)
        assert seconds == plain                                        # the same seconds as without the keyword
        assert pron == spy.expected(classes)
        assert [[d["class"] for d in row] for row in pron] == lists
        frames = model.align(audios, labels, use_ctc=use_ctc, return_pronunciation=True, pronunciation_classes=40, return_frames=True)
        assert len(frames) == 9 and frames[4].shape == (4, 11, 5) and frames[5].dtype == torch.float64 and frames[7].dtype == torch.int32
        for b, row in enumerate(pron):
            for n, d in enumerate(row):
                assert d["rank"] == int(frames[7][b, n]) and d["frames"] == int(frames[8][b, n]) == int(frames[1][b, n] - frames[0][b, n])
        # with a confidence keyword and per_clip: the pronunciation list stays the last element
        sec_c, scores, pron_c = model.align(audios, labels, use_ctc=use_ctc, return_confidence=True, return_pronunciation=True,
                                            pronunciation_classes=40)
        assert sec_c == plain and pron_c == spy.expected(classes) and set(scores[0]) >= {"occupancy"}
        sec_p, pron_p = model.align(audios, labels, use_ctc=use_ctc, per_clip=True, return_pronunciation=True, pronunciation_classes=40,
                                    pronunciation_top_k=2)
        assert sec_p == model.align(audios, labels, use_ctc=use_ctc, per_clip=True) and pron_p == spy.expected(classes)
        print(f"use_ctc={use_ctc}: ranks of clip 0 {[d['rank'] for d in pron[0]]}, gop {[round(d['gop'], 3) for d in pron[0]]}")


def test_the_sheet_functions_name_syllables(tiny):
    from lyricalignment_amd.harness import PinyinClassLUT, align_record_lines, align_song, suspect_characters
    model, tr = tiny["model"], tiny["tr"]
    lut = PinyinClassLUT([str(i) for i in range(403)], {str(i): i for i in range(403)})       # token id -> the same class id; 402 syllables
    ids_all = [int(v) for v in tr._clip_labels(0)[0]]                  # 11 labels: lines of 3 / 4 / 2 / 2
    lines = ["".join(chr(0x4E00 + 11 * k + j) for j in range(n)) for k, n in enumerate((3, 4, 2, 2))]
    ids, pos = {}, 0
    for line in lines:
        ids[line] = ids_all[pos: pos + len(line)]
        pos += len(line)
    with torch.no_grad():
        old = align_record_lines(model, tr._clip(0), lines, [False] * 4, lut, lambda t: ids[t])
        got, pron = align_record_lines(model, tr._clip(0), lines, [False] * 4, lut, lambda t: ids[t], with_pronunciation=True, top_k=3)
        (song, conf), pron_song = align_song(model, tr._clip(0), lines, lut, lambda t: ids[t], with_pronunciation=True, top_k=3)
    assert got == old == song and [len(line) for line in pron] == [3, 4, 2, 2] and "sung" in conf
    flat = [d for line in pron for d in line]
    assert [d["class"] for d in flat] == ids_all and all(d["syllable"] == lut.syllable_of(d["class"]) and len(d["top"]) == 3 for d in flat)
    assert all(isinstance(s, str) and v <= 0.0 for d in flat for s, v in d["top"]) and pron_song == pron
    assert suspect_characters(pron) == [(i, j, d["top"][0][0], d["gop"]) for i, line in enumerate(pron) for j, d in enumerate(line) if d["rank"] > 0]
