"""The alignment DP with optional lyric lines on the device (la_viterbi_spans_batch, ops.viterbi_spans_batch and the layers over it):
bit-for-bit against la_viterbi_batch without spans and against the float64 restatement tests/optional_spans_reference.py with them
(the restatement is pinned on the CPU by tests/test_host_optional_spans.py), then the Python surface on the tiny random-weight model of
tests/test_gpu_ragged.py."""
import numpy as np
import pytest
import torch

import optional_spans_reference as osr
from conftest import e2e_cases

pytestmark = pytest.mark.gpu


def _launch(ems, labels_list, skips, penalty, T_list=None):
    """Clips of different T / L in ONE launch -> host arrays (onset, offset, score, status)."""
    from lyricalignment_amd import ops
    B = len(ems)
    Lmax = max(max(len(l) for l in labels_list), 1)
    Tmax = max(e.shape[0] for e in ems)
    em = torch.zeros((B, Tmax, Lmax + 1), dtype=torch.float32)
    labels = torch.zeros((B, Lmax), dtype=torch.int32)
    skip = torch.full((B, Lmax + 1), -1, dtype=torch.int32)
    for b, (e, l, s) in enumerate(zip(ems, labels_list, skips)):
        em[b, : e.shape[0], : e.shape[1]] = torch.from_numpy(np.ascontiguousarray(e))
        labels[b, : len(l)] = torch.tensor(list(l), dtype=torch.int32)
        skip[b, : len(s)] = torch.tensor(list(s), dtype=torch.int32)
    n_labels = torch.tensor([len(l) for l in labels_list], dtype=torch.int32)
    n_frames = torch.tensor([e.shape[0] for e in ems] if T_list is None else T_list, dtype=torch.int32)
    on, off, score, status = ops.viterbi_spans_batch(em.cuda(), labels.cuda(), n_labels.cuda(), n_frames.cuda(), skip.cuda(), penalty)
    torch.cuda.synchronize()
    return on.cpu().numpy(), off.cpu().numpy(), score.cpu().numpy(), status.cpu().numpy()


def _assert_equals_reference(got, b, em, labels, skip, penalty, what):
    """Clip b of a launch against the float64 restatement: onset, offset, status and score exactly equal."""
    on, off, score, status = got
    L = len(labels)
    r_on, r_off, r_score, r_status, _ = osr.viterbi_spans(em, labels, skip, penalty)
    assert status[b] == r_status, what
    assert on[b, :L].tolist() == r_on and off[b, :L].tolist() == r_off, what
    assert (on[b, L:] == -1).all() and (off[b, L:] == -1).all(), what
    assert score[b] == r_score, (what, float(score[b]), r_score)                  # == on float64
    return r_on, r_status


# ------------------------------------------------------------------------------------------------ 1. no spans = la_viterbi_batch
@pytest.mark.parametrize("dpp", [1, 0])
def test_without_spans_equals_viterbi_batch_bit_for_bit(dpp):
    """conftest.e2e_cases() in one launch with every skip_from entry -1: frames, status and the float64 score of ops.viterbi_batch,
    under the DPP form and the LDS-exchange form of the one-wave kernel (the option is restored afterwards)."""
    from lyricalignment_amd import _lib, ops
    cases = list(e2e_cases())
    ems, labs = [c[2] for c in cases], [c[3].tolist() for c in cases]
    B, Lmax, Tmax = len(ems), max(len(l) for l in labs), max(e.shape[0] for e in ems)
    em = torch.zeros((B, Tmax, Lmax + 1), dtype=torch.float32)
    labels = torch.zeros((B, Lmax), dtype=torch.int32)
    for b, (e, l) in enumerate(zip(ems, labs)):
        em[b, : e.shape[0], : e.shape[1]] = torch.from_numpy(np.ascontiguousarray(e))
        labels[b, : len(l)] = torch.tensor(l, dtype=torch.int32)
    n_lab = torch.tensor([len(l) for l in labs], dtype=torch.int32).cuda()
    n_fr = torch.tensor([e.shape[0] for e in ems], dtype=torch.int32).cuda()
    em, labels = em.cuda(), labels.cuda()
    skip = torch.full((B, Lmax + 1), -1, dtype=torch.int32).cuda()
    before = _lib.get_option("viterbi_dpp")
    with _lib.option("viterbi_dpp", dpp):
        want = ops.viterbi_batch(em, labels, n_lab, n_fr)
        got = ops.viterbi_spans_batch(em, labels, n_lab, n_fr, skip)
        got_pen = ops.viterbi_spans_batch(em, labels, n_lab, n_fr, skip, 0.75)
        torch.cuda.synchronize()
    assert _lib.get_option("viterbi_dpp") == before
    assert (want[3] == 0).all()
    for name, w, g, gp in zip(("onset", "offset", "score", "status"), want, got, got_pen):
        assert torch.equal(w, g) and torch.equal(w, gp), name
    assert want[2].cpu().numpy().tobytes() == got[2].cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ 2. exact equality with the reference
def _random_case(seed, T, L, repeat_at=None, n_classes=50, lean=0.0):
    """Random emissions (equal classes share a column), labels with repeats, random spans of up to 8 labels at ~30 % of the end
    positions.  lean: label columns that much lower, so that leaving labels out pays and jumps are taken."""
    rs = np.random.RandomState(seed)
    lab = [int(v) for v in rs.randint(1, n_classes + 1, size=L)]
    if repeat_at is not None and 0 < repeat_at < L:
        lab[repeat_at] = lab[repeat_at - 1]
    lp = (-rs.rand(T, n_classes) * 4 - lean).astype(np.float32)
    ls = (-rs.rand(T, 1) * 4).astype(np.float32)
    em = np.concatenate([ls, lp[:, np.asarray(lab) - 1]], axis=1)
    skip = [-1] * (L + 1)
    for n in range(1, L + 1):
        if rs.rand() < 0.3:
            skip[n] = int(rs.randint(max(0, n - 8), n))
    return em, lab, skip


SHAPES = [                       # (T, L, clips, repeat_at, lean of the odd clips): what it exercises
    (1, 1, 3, None, 4.5), (2, 1, 3, None, 4.5),  # smallest cases
    (5, 4, 4, 2, 1.5),                           # equal-neighbour rule
    (60, 4, 4, 2, 1.5),                          # one wave: DPP shifts + bpermute
    (40, 31, 4, 7, 1.5),                         # 63 states: the last one-wave size
    (40, 32, 4, 7, 1.5),                         # 65 states: the first two-wave size
    (120, 100, 3, 50, 1.5),                      # 4 waves
    (600, 511, 2, 300, 1.5),                     # 16 waves, the label limit (masks in the workspace)
    (1800, 100, 2, 50, 4.5),                     # 4 waves, masks leave LDS for the workspace (18 frames per label: only a label column
]                                                # that is always below the silence column makes leaving a label out pay)


@pytest.mark.parametrize("T,L,clips,repeat_at,lean", SHAPES, ids=[f"T{s[0]}_L{s[1]}" for s in SHAPES])
def test_equals_the_float64_reference_exactly(T, L, clips, repeat_at, lean):
    """Onset, offset, status and score == the reference's for penalties 0 and 0.75; clips 0 and 1 carry the span (0, 1) when L == 1; odd clips
    have lean label columns.  From T = 2 on, some clip of the shape must actually take a jump."""
    from lyricalignment_amd import _lib
    cases = [_random_case(31 * T + L + 1000 * c, T, L, repeat_at, n_classes=3 if L <= 4 else 50, lean=lean * (c % 2)) for c in range(clips)]
    if L == 1:
        for c in cases[:2]:
            c[2][1] = 0                          # the only span L = 1 has: (0, 1), a span at position 0 that ends at L
    forms = [1, 0] if 2 * L + 1 <= 64 else [1]
    taken = 0
    for pen in (0.0, 0.75):
        for dpp in forms:
            with _lib.option("viterbi_dpp", dpp):
                got = _launch([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], pen)
            for b, (em, lab, skip) in enumerate(cases):
                r_on, r_status = _assert_equals_reference(got, b, em, lab, skip, pen, (T, L, b, pen, dpp))
                taken += r_status == osr.LA_OK and any(v < 0 for v in r_on)
    print(f"T={T} L={L}: {taken} (clip, penalty, form) runs report skipped labels")
    if T >= 2:
        assert taken > 0


def _planted(rs, labels, n_lines_of, present, gap):
    """tests/test_host_optional_spans.py's construction with class columns: 3 silence frames, 4 frames per character of a present line,
    `gap` silence frames between present lines, 3 silence frames; truth about -0.3 +- 0.1, the rest about -6 +- 1."""
    classes = sorted(set(labels))
    truth, pos, first = [0] * 3, 0, True
    for n_chars, here in zip(n_lines_of, present):
        if here:
            truth += [] if first else [0] * gap
            first = False
            for n in range(pos, pos + n_chars):
                truth += [1 + classes.index(labels[n])] * 4
        pos += n_chars
    truth += [0] * 3
    T = len(truth)
    cls = -6.0 + rs.randn(T, len(classes) + 1)
    cls[np.arange(T), truth] = -0.3 + 0.1 * rs.randn(T)
    cols = [0] + [1 + classes.index(v) for v in labels]
    return cls[:, cols].astype(np.float32)


def test_the_jump_arcs_that_must_work_are_taken_and_equal_the_reference():
    """Feasible clips in one launch whose best path provably uses: a span at position 0 (0..n), a span ending at L, two adjacent spans
    both taken, and a span whose J-1 arc is barred by equal labels (the path has to pass the silence J)."""
    from lyricalignment_amd.utils.alignment import spans_from_lines
    rs = np.random.RandomState(77)
    distinct = list(range(1, 13))
    lines = [3, 4, 3, 2]
    all_opt = spans_from_lines(lines, [True] * 4)
    plan = [("span at 0", distinct, all_opt, _planted(rs, distinct, lines, (0, 1, 1, 1), 2), [0, 1, 2]),
            ("span ending at L", distinct, all_opt, _planted(rs, distinct, lines, (1, 1, 1, 0), 0), [10, 11]),
            ("two adjacent spans", distinct, all_opt, _planted(rs, distinct, lines, (1, 0, 0, 1), 2), list(range(3, 10))),
            ("J-1 barred", [5, 6, 7, 5], [-1, -1, -1, 1, -1], _planted(rs, [5, 6, 7, 5], [1, 2, 1], (1, 0, 1), 0), [1, 2])]
    for pen in (0.0, 0.75):
        got = _launch([p[3] for p in plan], [p[1] for p in plan], [p[2] for p in plan], pen)
        for b, (what, lab, skip, em, gone) in enumerate(plan):
            r_on, r_status = _assert_equals_reference(got, b, em, lab, skip, pen, (what, pen))
            assert r_status == osr.LA_OK and [n for n, v in enumerate(r_on) if v < 0] == gone, what
    # the barred arc: label 3 (class 5) follows label 0 (class 5) with no silence frame planted between them: the path still never enters
    # state 7 from state 1; it spends a frame in the silence before the span (state 2) or in the one before label 3 (state 6)
    path = osr.viterbi_spans(plan[3][3], plan[3][1], plan[3][2], 0.0)[4]
    t = path.index(7)
    assert path[t - 1] in (2, 6) and osr.jump_sources(plan[3][1], plan[3][2])[1][7] is False


# ------------------------------------------------------------------------------------------------ 3. one ragged launch
def test_ragged_launch_with_empty_infeasible_and_out_of_range_entries():
    """Six clips of different T_b and L_b in one launch: an L = 0 clip (LA_EEMPTY), a clip too short for its mandatory labels
    (LA_EINFEASIBLE), and a clip whose skip_from holds out-of-range values (-7, n itself, n + 1, 2**30, INT32_MIN) beside its twin
    with -1: the values are ignored, not used as an index."""
    from lyricalignment_amd import _lib
    a = _random_case(1, 50, 9, 4, lean=1.5)
    b = _random_case(2, 23, 17, 5)
    c = _random_case(3, 3, 6, None)
    c = (c[0], c[1], [-1, -1, 1, -1, -1, -1, -1])           # 6 labels, one of them optional, 3 frames
    d = _random_case(4, 31, 5, None, lean=1.5)
    clean = [v if 0 <= v < n else -1 for n, v in enumerate(d[2])]
    junk = list(clean)
    fill = [-7, None, None, 2 ** 30, -2 ** 31]
    k = 0
    for n in range(len(junk)):
        if junk[n] < 0:
            v = fill[k % len(fill)]
            junk[n] = (n if k % 2 else n + 1) if v is None else v
            k += 1
    assert k >= 2
    empty = (np.zeros((12, 1), np.float32), [], [-1])
    ems = [a[0], b[0], empty[0], c[0], d[0], d[0]]
    labs = [a[1], b[1], [], c[1], d[1], d[1]]
    skips = [a[2], b[2], [-1], c[2], junk, clean]
    for pen in (0.0, 0.75):
        got = _launch(ems, labs, skips, pen)
        on, off, score, status = got
        assert status[2] == _lib.LA_EEMPTY and (on[2] == -1).all() and (off[2] == -1).all()
        assert status[3] == _lib.LA_EINFEASIBLE
        for i in (0, 1, 3, 5):
            _assert_equals_reference(got, i, ems[i], labs[i], skips[i], pen, (i, pen))
        assert status[0] == status[1] == status[4] == status[5] == _lib.LA_OK
        assert on[4].tolist() == on[5].tolist() and off[4].tolist() == off[5].tolist() and score[4] == score[5]
    # the launch's frame counts on the device decide, not the padded buffer: the same clips with a shorter T_b for clip 0
    got = _launch(ems, labs, skips, 0.0, T_list=[37, 23, 12, 3, 31, 31])
    _assert_equals_reference(got, 0, ems[0][:37], labs[0], skips[0], 0.0, "T_b < Tmax")


def test_ops_wrapper_rejects_bad_arguments():
    from lyricalignment_amd import ops
    em = torch.zeros((2, 10, 5), dtype=torch.float32).cuda()
    lab = torch.ones((2, 4), dtype=torch.int32).cuda()
    n = torch.tensor([4, 4], dtype=torch.int32).cuda()
    t = torch.tensor([10, 10], dtype=torch.int32).cuda()
    skip = torch.full((2, 5), -1, dtype=torch.int32).cuda()
    with pytest.raises(ValueError):
        ops.viterbi_spans_batch(em, lab, n, t, skip[:, :4])
    with pytest.raises(ValueError):
        ops.viterbi_spans_batch(em, lab, n, t, skip.long())
    with pytest.raises(ValueError):
        ops.viterbi_spans_batch(em, lab, n, t, skip, -1.0)
    with pytest.raises(ValueError):
        ops.viterbi_spans_batch(em, lab, n, t, skip, float("nan"))
    with pytest.raises(NotImplementedError):
        ops.viterbi_spans_batch(torch.zeros((1, 4, 513), dtype=torch.float32).cuda(), torch.ones((1, 512), dtype=torch.int32).cuda(),
                                n[:1], t[:1], torch.full((1, 513), -1, dtype=torch.int32).cuda())


# ------------------------------------------------------------------------------------------------ 4. the Python surface on the tiny model
IDX = [0, 1, 3, 5]                                           # clips of tests/test_gpu_ragged.py: 11, 5, 8, 3 labels
SPANS = [[(0, 3), (3, 7)], [(3, 5)], [(2, 5)], []]


@pytest.fixture(scope="module")
def tiny():
    import test_gpu_ragged as tr
    from test_gpu_parity_full import _build
    model, _ = _build("tiny", torch.float32)
    return dict(model=model, audios=[tr._clip(i) for i in IDX], labels=tr._padded_labels(IDX), tr=tr)


@pytest.mark.parametrize("use_ctc", [True, False])
def test_align_with_spans_equals_the_two_step_route(tiny, use_ctc):
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels = tiny["model"], tiny["audios"], tiny["labels"]
    two = ua.perform_viterbi_ctc if use_ctc else ua.perform_viterbi
    with torch.no_grad():
        logits, _ = model.frame_manual_forward(audios)
        for pen in (0.0, 2.0):
            fused = model.align(audios, labels, use_ctc=use_ctc, optional_spans=SPANS, skip_penalty=pen)
            assert fused == two(logits, labels, optional_spans=SPANS, skip_penalty=pen)
            on, off, score, status = model.align(audios, labels, use_ctc=use_ctc, optional_spans=SPANS, skip_penalty=pen, return_frames=True)
            assert status.tolist() == [0] * 4
            for b, res in enumerate(fused):
                assert [None if r is None else round(r[0] / 0.02) for r in res] == [None if v < 0 else v for v in on[b, : len(res)].tolist()]
                gone = {n for n, r in enumerate(res) if r is None}
                assert gone == {n for a, e in SPANS[b] if res[a] is None for n in range(a, e)}      # whole spans, and only spans
            print(f"use_ctc={use_ctc} penalty={pen}: skipped labels per clip {[sum(r is None for r in res) for res in fused]}")
        plain = model.align(audios, labels, use_ctc=use_ctc)
        assert model.align(audios, labels, use_ctc=use_ctc, optional_spans=None) == plain
        assert model.align(audios, labels, use_ctc=use_ctc, optional_spans=[[], [], [], []]) == plain
        assert two(logits, labels, optional_spans=[[], [], [], []]) == two(logits, labels)


def test_per_clip_with_spans_equals_each_clip_alone_and_confidence_is_refused(tiny):
    model, audios, labels, tr = tiny["model"], tiny["audios"], tiny["labels"], tiny["tr"]
    with torch.no_grad():
        batch = model.align(audios, labels, per_clip=True, optional_spans=SPANS)
        for r, i in enumerate(IDX):
            alone = model.align([audios[r]], tr._clip_labels(i), per_clip=True, optional_spans=[SPANS[r]])
            assert batch[r] == alone[0], i
        with pytest.raises(ValueError):
            model.align(audios, labels, optional_spans=SPANS, return_confidence=True)
        with pytest.raises(ValueError):
            model.align(audios, labels, per_clip=True, optional_spans=SPANS, return_confidence=True)
        for bad in ([[(0, 12)], [], [], []], [[(2, 2)], [], [], []], [[(0, 3), (1, 3)], [], [], []], [[], [], []]):
            with pytest.raises(ValueError):
                model.align(audios, labels, optional_spans=bad)


def test_long_form_with_spans_equals_the_two_step_route(tiny):
    """A 33 s recording (two encoder chunks, 1650 frames) with 14 labels in four lines, two of them optional."""
    from lyricalignment_amd.utils import alignment as ua
    model, tr = tiny["model"], tiny["tr"]
    audio = np.concatenate([tr._clip(4), tr._clip(3)])
    labels = torch.from_numpy(np.random.RandomState(5).randint(2, 403, size=(1, 14)))
    spans = [[(3, 7), (10, 14)]]
    with torch.no_grad():
        logits, _ = model.frame_manual_forward([audio])
        assert logits.shape[1] > 1500
        assert model.align([audio], labels, optional_spans=spans) == ua.perform_viterbi_ctc(logits, labels, optional_spans=spans)


def test_align_record_lines_returns_none_for_exactly_the_skipped_lines(tiny):
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
    for pen in (0.0, 3.0):
        got = align_record_lines(model, tr._clip(0), lines, optional, lut, lambda t: ids[t], use_ctc_loss=True, skip_penalty=pen)
        with torch.no_grad():
            chars = model.align([tr._clip(0)], tr._clip_labels(0), use_ctc=True, optional_spans=spans, skip_penalty=pen)[0]
        assert len(got) == 4
        pos = 0
        for line, entry in zip(lines, got):
            part = chars[pos: pos + len(line)]
            pos += len(line)
            if entry is None:
                assert all(c is None for c in part)
            else:
                assert entry == [[c[0], c[1], ch] for c, ch in zip(part, line)]
        assert got[2] is not None
        print(f"penalty {pen}: lines left out {[i for i, e in enumerate(got) if e is None]}")
    with pytest.raises(ValueError):
        align_record_lines(model, tr._clip(0), lines, optional, lut, lambda t: ids[t][:-1])
