"""Off-sheet slots on the device (csrc/la_offsheet.hip: la_emissions_offsheet_columns writes log P(frame is not silence) - penalty into
the slots' columns of the compact emission matrix; ops.offsheet_columns; the `off_sheet` / `off_sheet_penalty` / `return_off_sheet`
keywords of perform_viterbi(_ctc)*, AlignModel.align and the sheet functions).
1. the kernel against the float64 formula of tests/offsheet_reference.py: every written value equal or adjacent in float32 (the
   device's log / expm1 may differ from numpy's in the last float64 bits), every other cell untouched, two calls and a clip alone bit-equal;
2. the lattice on the device's own post-kernel matrix: onset, offset, status and score bit-equal to the float64 restatements on the
   expanded lattice, the posteriors within the project's bound 8 T 2^-23 max(1, value) of the float64 yardstick;
3. the public surface on a tiny model: the fused call equals the two-step route, and without the keyword nothing changes."""
import math

import numpy as np
import pytest
import torch

import offsheet_reference as osr
import readings_reference as rdr
import repeat_posterior_reference as rpr
from test_gpu_repeat_spans import _planted_logits


def _planted(segments, T, width):
    """_planted_logits with the segments placed by hand: [(class, first frame, last frame + 1), ...] -- neighbours may touch -- and a
    silence logit of -12 on sung frames: silence (log-probability -12) is then dearer there than a wrong character (about -10), as on
    real singing, so that without a slot a character is stretched over an off-sheet passage."""
    lg = torch.full((1, T, width), -4.0)
    lg[:, :, -1] = 6.0
    for c, t, u in segments:
        lg[0, t:u, c] = 6.0
        lg[0, t:u, -1] = -12.0
    return lg


pytestmark = pytest.mark.gpu
HOP = 0.02
LN100 = math.log(100.0)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 1. the kernel
LABELS = 70                                                     # L': label columns of the window
SPECIAL = np.array([0.0, -6e-8, -1e-3, -0.69, -5.0, -50.0, -999.0, -1000.0], dtype=np.float32)
SLOTS = [[], [37], [0] + list(range(3, 66)) + [69]]             # 0, 1 and 65 slots (more than one wave); the first and the last column


def kernel_case(frames):
    """-> (wide host matrix [3, Tmax + 2, 3 + L' + 1 + 3] of sentinels with the silence column filled, slot_cols, n_slots, n_frames)."""
    rs = np.random.RandomState(11 + sum(frames))
    Tmax = max(frames)
    wide = (rs.rand(3, Tmax + 2, LABELS + 7) * -30.0 - 1.0).astype(np.float32)
    sil = (-rs.rand(3, Tmax + 2) * 20.0).astype(np.float32)
    sil[np.abs(sil) < 1e-30] = -1.0                             # no subnormals
    for b in range(3):
        sil[b, : len(SPECIAL)] = np.roll(SPECIAL, -b)             # the first rows: the edge values, in another order per clip
    wide[:, :, 3] = sil
    cols = np.full((3, 67), -1, dtype=np.int32)                 # a row pitch beyond the widest list
    for b, s in enumerate(SLOTS):
        cols[b, : len(s)] = s
    return wide, cols, np.array([len(s) for s in SLOTS], np.int32), np.array(frames, np.int32)


def _run(wide, cols, n_slots, n_frames, penalty, clips=slice(None)):
    from lyricalignment_amd import ops
    Tmax = int(max(n_frames))
    dev = torch.from_numpy(wide[clips].copy()).cuda()
    em = dev[:, :Tmax, 3: 3 + LABELS + 1]                       # a column window: row stride > L' + 1, a batch stride that is not T * row stride
    assert em.stride(1) == LABELS + 7 and em.stride(0) == (Tmax + 2) * (LABELS + 7)
    out = ops.offsheet_columns(em, torch.from_numpy(cols[clips]).cuda(), torch.from_numpy(n_slots[clips]).cuda(),
                               torch.from_numpy(n_frames[clips]).cuda(), penalty)
    assert out is em
    return dev.cpu().numpy()


@pytest.mark.parametrize("penalty", [0.0, LN100, 2000.0], ids=["0", "ln100", "2000"])
@pytest.mark.parametrize("frames", [(0, 1, 7), (63, 65, 257)], ids=["T0_1_7", "T63_65_257"])
def test_the_kernel_writes_the_formula_into_the_slot_columns_and_nothing_else(frames, penalty):
    wide, cols, n_slots, n_frames = kernel_case(frames)
    got = _run(wide, cols, n_slots, n_frames, penalty)
    want, written = wide.copy(), np.zeros(wide.shape, dtype=bool)
    for b, s in enumerate(SLOTS):
        want[b, :, 3:] = osr.write_columns(wide[b, :, 3:], s, frames[b], penalty)
        for x in s:
            written[b, : frames[b], 3 + 1 + x] = True
    assert written.sum() == sum(len(s) * t for s, t in zip(SLOTS, frames))
    # every cell that must not be written keeps its bits: other columns, the silence column, rows at or beyond n_frames, the clip without
    # slots, the guard columns on both sides and the guard rows behind
    assert _same_bits(got[~written], wide[~written])
    g, w = got[written], want[written]
    assert osr.adjacent_or_equal(g, w).all(), (g[~osr.adjacent_or_equal(g, w)][:5], w[~osr.adjacent_or_equal(g, w)][:5])
    share = float((g == w).mean()) if g.size else 1.0
    print(f"frames={frames} penalty={penalty:.3f}: {g.size} written values, exactly equal to the float64 formula: {share:.6f}")
    if penalty == 2000.0:
        assert (g == -1000.0).all()                             # the floor everywhere
    else:
        assert (g > -1000.0).any() and (g == -1000.0).any()     # silence 0 gives the floor, everything else a value
    # two calls agree bit for bit, and a clip alone equals the same clip in the batch
    assert _same_bits(_run(wide, cols, n_slots, n_frames, penalty), got)
    for b in range(3):
        alone = _run(wide, cols, n_slots, n_frames, penalty, clips=slice(b, b + 1))
        assert _same_bits(alone[0], got[b]), b


def test_entries_outside_the_label_columns_are_skipped():
    from lyricalignment_amd import ops
    wide, cols, n_slots, n_frames = kernel_case((63, 65, 257))
    bad = cols.copy()
    bad[1, :3] = [-5, 37, LABELS]                                # two entries outside 0 .. L'-1 around the good one
    n_bad = n_slots.copy()
    n_bad[1] = 3
    assert _same_bits(_run(wide, bad, n_bad, n_frames, LN100), _run(wide, cols, n_slots, n_frames, LN100))
    em = torch.zeros((1, 4, 5)).cuda()
    one = torch.zeros((1,), dtype=torch.int32).cuda()
    for penalty in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="penalty"):
            ops.offsheet_columns(em, one[:, None], one, one, penalty)


# ------------------------------------------------------------------------------------------------ 2. the lattice
def _bound(T, ref):
    return 8 * T * 2.0 ** -23 * np.maximum(1.0, np.abs(ref))


class _Case:
    """One clip through the product's pieces up to the lattice: the prep on the expanded rows (with alternatives: the fold), the kernel,
    then run_lattice -- and the float64 restatement on the device's own post-kernel matrix."""

    def __init__(self, pred, labels, slots, penalty=LN100, spans=(), skip_penalty=0.0, repeats=None, repeat_penalty=0.0, anchors=(), alts=None):
        from lyricalignment_amd import _lib, ops
        from lyricalignment_amd.utils import alignment as ua
        self.T, self.labels, self.slots = pred.shape[1], labels, slots
        self.kw = dict(off_sheet=[slots], off_sheet_penalty=penalty, skip_penalty=skip_penalty)
        if spans:
            self.kw["optional_spans"] = [list(spans)]
        if repeats is not None:
            self.kw.update(repeat_spans=[list(repeats)], repeat_penalty=repeat_penalty)
        if anchors:
            self.kw["onset_anchors"] = [list(anchors)]
        if alts:
            self.kw["alternatives"] = [list(alts)]
        off = ua._off_sheet_of("t", [slots], penalty, [labels], [list(spans)], None if repeats is None else [list(repeats)], None, [list(anchors)],
                               None if alts is None else [list(alts)])
        sheet = self.sheet = osr.Sheet(labels, slots)
        lab, n_lab, lists = ua._labels_to_device(off.label_lists, 1, pred.device)
        nf = torch.tensor([self.T], dtype=torch.int32).cuda()
        prep = lambda lab_x, n_x: ops.emissions_from_logits(pred, lab_x, n_x, _lib.LA_VARIANT_CTC)
        ids = sheet.ids
        if alts:
            rd = ua._readings_of(off.alternatives, lists)
            em = ua.readings_route(rd, prep, n_lab, nf, pred.device).em
            ids = [osr.OFF_SHEET_ID if p in sheet.slot_pos.values() else v for p, v in enumerate(rdr.lattice_ids(rd.sets[0]))]
            assert off.ids_with_slots(rd.lattice_ids)[0, : sheet.L].tolist() == ids
        else:
            em = prep(lab, n_lab)
        floor = em[0, :, [1 + p for p in sheet.slot_pos.values()]].cpu().numpy()
        assert (floor == -1000.0).all()                           # class 0: the provider writes the floor, the kernel overwrites it
        ops.offsheet_columns(em, off.slot_cols.cuda(), off.n_slots.cuda(), nf, penalty)
        self.em = em[0].cpu().numpy()
        self.skip = sheet.skip_from(spans)
        self.rf = None if repeats is None else sheet.repeat_from(repeats)
        self.lo = self.hi = None
        windows = None
        if anchors:
            self.lo, self.hi = ua.windows_from_anchors(sheet.L, self.T, None, sheet.indexed(anchors), HOP)
            windows = ua._windows_of(None, off.onset_anchors, lists, [self.T], HOP)
        self.ids, self.skip_penalty, self.repeat_penalty = ids, skip_penalty, repeat_penalty
        self.r = ua.run_lattice(em, torch.tensor([ids], dtype=torch.int32).cuda(), n_lab, nf, ua._skip_from_of_spans(off.optional_spans, lists),
                                windows, skip_penalty, None, 2, None, None if repeats is None else ua._repeat_from_of_spans(off.repeat_spans, lists),
                                repeat_penalty)
        self.ref = osr.viterbi(self.em, ids, self.skip, skip_penalty, self.lo, self.hi, self.rf, repeat_penalty)

    def assert_bit_equal(self):
        on, off, score, status, path = self.ref
        r = self.r
        assert r.onset[0, : self.sheet.L].tolist() == list(on) and r.offset[0, : self.sheet.L].tolist() == list(off)
        assert int(r.status[0]) == status == 0
        assert np.float64(r.score[0].item()).tobytes() == np.float64(score).tobytes(), (r.score[0].item(), score)
        if r.path is not None:
            assert r.path[0, : self.T].tolist() == list(path)

    def seconds(self):
        on, off = self.ref[0], self.ref[1]
        return [None if on[p] < 0 else [float(on[p]) * HOP, float(off[p]) * HOP] for p in self.sheet.label_pos]

    def heard(self):
        on, off, path = self.ref[0], self.ref[1], self.ref[4]
        if self.rf is not None:
            visits = self.sheet.slot_visits(path)
        else:
            visits = sorted(((n, on[p], off[p]) for n, p in self.sheet.slot_pos.items() if on[p] >= 0), key=lambda v: v[1])
        return [{"position": n, "onset": float(t) * HOP, "offset": float(u) * HOP, "frames": u - t} for n, t, u in visits]


def _noisy(lg, seed, scale=0.3):
    return (lg + torch.from_numpy(np.random.RandomState(seed).randn(*lg.shape).astype(np.float32)) * scale).cuda()


def test_slots_only_take_the_planted_passages_bit_for_bit():
    from lyricalignment_amd.utils import alignment as ua
    labels = [4, 3, 9, 6]                      # sung: 4 3 | 11 8 (off the sheet, right between the 3 and the 9) | 9 6 | 2 (off the sheet, behind the 6)
    pred = _noisy(_planted([(4, 5, 10), (3, 15, 20), (11, 20, 25), (8, 25, 30), (9, 30, 35), (6, 40, 45), (2, 45, 50)], 60, 14), 1)
    case = _Case(pred, labels, [0, 2, 4])
    case.assert_bit_equal()
    heard = case.heard()
    assert [(h["position"], round(h["onset"] / HOP), h["frames"]) for h in heard] == [(2, 20, 10), (4, 45, 5)]       # the slot before label 0 is unused
    assert [(round(s[0] / HOP), round(s[1] / HOP)) for s in case.seconds()] == [(5, 10), (15, 20), (30, 35), (40, 45)]
    seconds, got = ua.perform_viterbi_ctc(pred, torch.tensor([labels]), return_off_sheet=True, **case.kw)
    assert seconds == [case.seconds()] and got == [heard]
    assert ua.perform_viterbi_ctc(pred, torch.tensor([labels]), **case.kw) == seconds
    # without slots the neighbouring characters are stretched over the first passage (silence is dearer there than a wrong character)
    plain = ua.perform_viterbi_ctc(pred, torch.tensor([labels]))[0]
    assert round((plain[1][1] - plain[1][0] + plain[2][1] - plain[2][0]) / HOP) == 20 and plain != seconds[0]
    assert ua.perform_viterbi_ctc(pred, torch.tensor([labels]), return_off_sheet=True) == ([plain], [[]])


def test_an_optional_line_with_a_slot_inside_it():
    from lyricalignment_amd.utils import alignment as ua
    labels = [4, 3, 9, 6, 7, 2]                                        # lines (4 3) (9 6) (7 2); line two may be absent and has a slot inside
    for sung, line_two in (([4, 3, 9, 12, 6, 7, 2], True), ([4, 3, 12, 7, 2], False)):
        pred = _noisy(_planted_logits(sung, 5 * (2 * len(sung) + 1), 14, 5), 2)
        case = _Case(pred, labels, [2, 3, 4], spans=[(2, 4)], skip_penalty=0.25)
        assert case.sheet.expanded == [4, 3, 0, 9, 0, 6, 0, 7, 2] and case.skip == [-1, -1, -1, 2, -1, 4, 3, 6, -1, -1]
        case.assert_bit_equal()
        seconds, got = ua.perform_viterbi_ctc(pred, torch.tensor([labels]), return_off_sheet=True, **case.kw)
        assert seconds == [case.seconds()] and got == [case.heard()]
        assert (seconds[0][2] is not None) == line_two and (seconds[0][3] is not None) == line_two
        # sung: the slot inside the line takes the 12; not sung: the line goes with its slot, and a slot at either edge takes the 12
        assert len(got[0]) == 1 and got[0][0]["position"] in ((3,) if line_two else (2, 4)) and got[0][0]["frames"] == 5


def test_slots_with_anchors():
    from lyricalignment_amd.utils import alignment as ua
    labels = [4, 3, 9, 6]
    pred = _noisy(_planted_logits([4, 3, 11, 8, 9, 6], 5 * 13, 14, 5), 3)
    case = _Case(pred, labels, [2, 4], anchors=[(2, 45 * HOP, 3 * HOP), (0, 5 * HOP, 0.1)])
    case.assert_bit_equal()
    seconds, got = ua.perform_viterbi_ctc(pred, torch.tensor([labels]), return_off_sheet=True, **case.kw)
    assert seconds == [case.seconds()] and got == [case.heard()] and [h["position"] for h in got[0]] == [2]
    assert abs(seconds[0][2][0] - 45 * HOP) <= 3 * HOP + 1e-9


def test_slots_with_a_repeat_span_and_segments():
    from lyricalignment_amd.utils import alignment as ua
    labels = [3, 5, 7, 2, 9, 4]                                        # lines (3 5) (7 2) (9 4); sung A B B C with an ad-lib inside the first B
    pred = _noisy(_planted_logits([3, 5, 7, 12, 2, 7, 2, 9, 4], 5 * 19, 14, 5), 4)
    case = _Case(pred, labels, [3, 6], repeats=[(2, 4)], repeat_penalty=1.0)
    assert case.sheet.expanded == [3, 5, 7, 0, 2, 9, 4, 0] and case.rf == [-1, -1, 5, -1, -1, -1, -1, -1]      # the slot inside the line repeats with it
    case.assert_bit_equal()
    seconds, segments, got = ua.perform_viterbi_ctc(pred, torch.tensor([labels]), return_segments=True, return_off_sheet=True, **case.kw)
    assert seconds == [case.seconds()] and got == [case.heard()]
    assert [(h["position"], h["frames"]) for h in got[0]] == [(3, 5)]    # used on the first pass, skipped on the second
    back = {p: n for n, p in enumerate(case.sheet.label_pos)}
    assert segments == [[(back[p], t * HOP, u * HOP) for p, t, u in osr.rr.segments(case.ref[4]) if p in back]]
    assert [n for n, _, _ in segments[0]] == [0, 1, 2, 3, 2, 3, 4, 5]


def test_slots_with_alternatives():
    from lyricalignment_amd.utils import alignment as ua
    labels = [4, 3, 9, 6]                                              # the sheet says 3 where 7 is sung; an off-sheet 12 before the 9
    pred = _noisy(_planted_logits([4, 7, 12, 9, 6], 5 * 11, 14, 5), 5)
    case = _Case(pred, labels, [2, 4], alts=[(1, [7]), (2, [5])])
    case.assert_bit_equal()
    seconds, readings, got = ua.perform_viterbi_ctc(pred, torch.tensor([labels]), return_readings=True, return_off_sheet=True, **case.kw)
    assert seconds == [case.seconds()] and got == [case.heard()] and [h["position"] for h in got[0]] == [2]
    assert [r[0] for r in readings[0]] == [4, 7, 9, 6] and len(readings[0]) == 4


def test_a_wide_sheet_takes_the_strip_kernel():
    from lyricalignment_amd.utils import alignment as ua
    rs = np.random.RandomState(6)
    T, L, V = 560, 510, 40                                             # 510 labels + 6 slots = 516 expanded labels
    labels = [int(v) for v in rs.randint(1, V + 1, size=L)]
    pred = torch.from_numpy((rs.randn(1, T, V + 2) * 2.0).astype(np.float32)).cuda()
    case = _Case(pred, labels, [0, 100, 200, 300, 400, 510], penalty=1.0)
    assert case.sheet.L == 516 and case.r.path is None
    case.assert_bit_equal()
    seconds, got = ua.perform_viterbi_ctc(pred, torch.tensor([labels]), return_off_sheet=True, **case.kw)
    assert seconds == [case.seconds()] and got == [case.heard()]
    with pytest.raises(NotImplementedError, match="511"):
        ua.perform_viterbi_ctc_scored(pred, torch.tensor([labels]), **case.kw)


@pytest.mark.parametrize("kind", ["span", "sheet", "song"])
def test_the_posteriors_stay_within_the_bound_of_the_float64_yardstick(kind):
    from lyricalignment_amd.utils import alignment as ua
    labels = [4, 3, 9, 6, 7, 2]
    sung, slots = ([4, 3, 12, 9, 6, 7, 2], [0, 2, 4]) if kind != "song" else ([4, 3, 9, 12, 6, 9, 6, 7, 2], [0, 3, 4])      # song: a slot inside the repeat
    pred = _noisy(_planted_logits(sung, 5 * (2 * len(sung) + 1), 14, 5) * 0.5, 7, 0.5)          # soft enough for posteriors inside (0, 1)
    spans, repeats = [(4, 6)], ([(2, 4)] if kind == "song" else None)
    # penalty 2: on the soft logits silence costs about 3 nats on a sung frame, so that the slot (2) and not the silence takes the 12
    case = _Case(pred, labels, slots, penalty=2.0, spans=spans, skip_penalty=0.25, repeats=repeats, repeat_penalty=0.5)
    f = {"span": ua.perform_viterbi_ctc_scored, "sheet": ua.perform_viterbi_ctc_sheet_scored, "song": ua.perform_viterbi_ctc_song_scored}[kind]
    seconds, scores, heard = f(pred, torch.tensor([labels]), return_off_sheet=True, **case.kw)
    assert seconds == [case.seconds()] and heard == [case.heard()]
    d, sheet, T = scores[0], case.sheet, case.T
    ref = rpr.posteriors(case.em, case.ids, case.skip, 0.25, case.rf, 0.5)
    occ, onp, offp = (np.asarray(v) for v in rpr.scores(ref, case.ref[0], case.ref[1], 2))
    worst = 0.0

    def close(got, want, what):
        nonlocal worst
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        worst = max(worst, float((np.abs(got - want) / _bound(T, want)).max()))
        assert (np.abs(got - want) <= _bound(T, want)).all(), (what, got, want)

    keep = sheet.label_pos
    close(d["occupancy"], occ[keep], "occupancy")
    close(d["onset_prob"], onp[keep], "onset_prob")
    close(d["offset_prob"], offp[keep], "offset_prob")
    close(d["visits" if kind == "song" else "sung_prob"], ref["visits"][keep], "sung_prob")
    ends = [e for _, e in sheet.optional_spans(spans)]
    close(d["span_skip_prob"], ref["span_skip"][ends[:1]], "span_skip_prob")
    assert list(d["off_sheet_prob"]) == slots
    slot_p = [sheet.slot_pos[n] for n in slots]
    close(list(d["off_sheet_prob"].values()), ref["visits"][slot_p], "off_sheet_prob")
    if kind != "song":             # a slot is used or skipped: the DEVICE's own two numbers sum to one (the public dicts keep only the caller's
        # spans, so the sweep is asked once more, through run_lattice on the same matrix: present_prob at the slot + the skip of its span)
        c = case
        r = ua.run_lattice(torch.from_numpy(c.em)[None].cuda(), torch.tensor([c.ids], dtype=torch.int32).cuda(), torch.tensor([sheet.L], dtype=torch.int32).cuda(),
                           torch.tensor([T], dtype=torch.int32).cuda(), torch.tensor([c.skip], dtype=torch.int32), None, 0.25, kind, 2)
        used, skipped = r.present_prob[0, slot_p].cpu().numpy().astype(np.float64), r.span_skip_prob[0, ends[1:]].cpu().numpy().astype(np.float64)
        assert used.astype(np.float32).tolist() == [np.float32(v) for v in d["off_sheet_prob"].values()]       # what the dict reports
        close(used + skipped, np.ones(3), "off_sheet_prob + the skip probability of the slot's own span")
        close(skipped, ref["span_skip"][ends[1:]], "the slots' span_skip_prob")
    assert min(d["off_sheet_prob"].values()) < max(d["off_sheet_prob"].values()) and max(d["off_sheet_prob"].values()) > 0.5       # one slot is used
    print(f"{kind}: largest |device - float64| over the bound 8 T 2^-23 max(1, value): {worst:.4f}")


# ------------------------------------------------------------------------------------------------ 3. the public surface
@pytest.fixture(scope="module")
def tiny():
    import test_gpu_ragged as tr
    from test_gpu_parity_full import _build
    model, _ = _build("tiny", torch.float32)
    idx = [0, 1, 3, 5]                                           # clips of tests/test_gpu_ragged.py: 11, 5, 8, 3 labels
    return dict(model=model, audios=[tr._clip(i) for i in idx], labels=tr._padded_labels(idx), tr=tr, idx=idx)


OFF = [[0, 4, 11], [2], [], [0, 3]]


@pytest.mark.parametrize("use_ctc", [True, False])
def test_align_equals_the_two_step_route_and_nothing_changes_without_the_keyword(tiny, monkeypatch, use_ctc):
    from lyricalignment_amd import ops
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels = tiny["model"], tiny["audios"], tiny["labels"]
    two = ua.perform_viterbi_ctc if use_ctc else ua.perform_viterbi
    sheet = ua.perform_viterbi_ctc_sheet_scored if use_ctc else ua.perform_viterbi_sheet_scored
    calls = []
    real = ops.offsheet_columns
    monkeypatch.setattr(ops, "offsheet_columns", lambda *a: calls.append(a) or real(*a))
    with torch.no_grad():
        logits, _ = model.frame_manual_forward(audios)
        plain = model.align(audios, labels, use_ctc=use_ctc)
        assert model.align(audios, labels, use_ctc=use_ctc, off_sheet=None) == plain
        assert model.align(audios, labels, use_ctc=use_ctc, off_sheet=[[], [], [], []], off_sheet_penalty=0.5) == plain
        assert model.align(audios, labels, use_ctc=use_ctc, off_sheet=[[], [], [], []], return_off_sheet=True) == (plain, [[], [], [], []])
        assert not calls                                               # without slots the call never heard of the kernel
        for kw in (dict(), dict(off_sheet_penalty=0.0), dict(optional_spans=[[(7, 9)], [], [(5, 8)], []], skip_penalty=0.25),
                   dict(repeat_spans=[[(3, 7)], [(0, 5)], [], []], return_segments=True)):
            fused = model.align(audios, labels, use_ctc=use_ctc, off_sheet=OFF, return_off_sheet=True, **kw)
            other = two(logits, labels, off_sheet=OFF, return_off_sheet=True, **kw)
            assert fused == other and len(fused) == (3 if "return_segments" in kw else 2), kw
            assert [len(s) for s in fused[0]] == [11, 5, 8, 3] and fused[-1][2] == []
            assert all(h["position"] in OFF[b] and h["frames"] == round((h["offset"] - h["onset"]) / HOP) for b, c in enumerate(fused[-1]) for h in c)
            if kw.get("off_sheet_penalty") == 0.0:                     # at penalty 0 a slot beats every character on every voiced frame: slots are used
                assert all(bool(c) == bool(OFF[b]) for b, c in enumerate(fused[-1])), fused[-1]
        assert len(calls) == 8
        seconds, scores, heard = model.align(audios, labels, use_ctc=use_ctc, off_sheet=OFF, return_off_sheet=True, return_sheet_confidence=True)
        s2, sc2, h2 = sheet(logits, labels, off_sheet=OFF, return_off_sheet=True)
        assert seconds == s2 and heard == h2 and [list(d["off_sheet_prob"]) for d in scores] == OFF
        T = logits.shape[1]                                   # the two routes' scores: the bound tests/test_gpu_readings.py holds them to
        for d, e in zip(scores, sc2):
            diff = max((abs(a - b) for a, b in zip(d["off_sheet_prob"].values(), e["off_sheet_prob"].values())), default=0.0)
            print(f"use_ctc={use_ctc}: off_sheet_prob, fused against two-step: max |difference| {diff:.3e} (bound {8 * T * 2.0 ** -23:.3e})")
            assert diff <= 8 * T * 2.0 ** -23
            assert len(d["occupancy"]) == len(d["sung_prob"]) == len(e["occupancy"])
        # per_clip: the two-step route on the per-clip logits with n_frames, and each clip as if alone
        batch = model.align(audios, labels, use_ctc=use_ctc, per_clip=True, off_sheet=OFF, return_off_sheet=True)
        lg = model.frame_logits_per_clip(audios)
        pad = torch.zeros((len(lg), max(t.shape[0] for t in lg), lg[0].shape[1]), dtype=torch.float32, device=lg[0].device)
        for r, t in enumerate(lg):
            pad[r, : t.shape[0]] = t
        assert batch == two(pad, labels, n_frames=[t.shape[0] for t in lg], off_sheet=OFF, return_off_sheet=True)
        for r, i in enumerate(tiny["idx"]):
            alone = model.align([audios[r]], tiny["tr"]._clip_labels(i), use_ctc=use_ctc, per_clip=True, off_sheet=[OFF[r]], return_off_sheet=True)
            assert (batch[0][r], batch[1][r]) == (alone[0][0], alone[1][0]), i
        print(f"use_ctc={use_ctc}: slot visits {[[(h['position'], h['frames']) for h in c] for c in fused[-1]]}")


def test_pronunciation_the_long_form_and_the_sheet_functions(tiny):
    from lyricalignment_amd import _lib
    from lyricalignment_amd.harness import PinyinClassLUT, align_record_lines, align_record_lrc, align_song
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels, tr = tiny["model"], tiny["audios"], tiny["labels"], tiny["tr"]
    with torch.no_grad():
        # with return_pronunciation the slot entries carry `top` and the per-character dicts are those of the same expanded lattice
        logits, _ = model.frame_manual_forward(audios)
        seconds, pron, heard = model.align(audios, labels, off_sheet=OFF, off_sheet_penalty=0.5, return_off_sheet=True, return_pronunciation=True,
                                           pronunciation_classes=40, pronunciation_top_k=3)
        s2, p2, h2 = ua.perform_viterbi_ctc(logits, labels, off_sheet=OFF, off_sheet_penalty=0.5, return_off_sheet=True, return_pronunciation=True,
                                            pronunciation_classes=40, pronunciation_top_k=3)
        assert seconds == s2 == model.align(audios, labels, off_sheet=OFF, off_sheet_penalty=0.5)
        assert [len(row) for row in pron] == [11, 5, 8, 3] and any(heard)
        lists = [[int(v) for v in row if int(v) != -100] for row in labels]
        assert [[d["class"] for d in row] for row in pron] == lists == [[d["class"] for d in row] for row in p2]
        for c, c2 in zip(heard, h2):
            assert [(h["position"], h["frames"]) for h in c] == [(h["position"], h["frames"]) for h in c2]
            assert all(len(h["top"]) == 3 and all(cls >= 1 and s <= 0.0 for cls, s in h["top"]) for h in c)
            assert all(h["top"][0][1] >= h["top"][1][1] >= h["top"][2][1] for h in c)
        # the long form: 33 s, two encoder chunks
        audio = np.concatenate([tr._clip(4), tr._clip(3)])
        lab = torch.from_numpy(np.random.RandomState(5).randint(2, 403, size=(1, 14)))
        kw = dict(off_sheet=[[0, 7, 14]], off_sheet_penalty=0.5, return_off_sheet=True, optional_spans=[[(10, 14)]])
        long_logits, _ = model.frame_manual_forward([audio])
        assert long_logits.shape[1] > 1500
        assert model.align([audio], lab, **kw) == ua.perform_viterbi_ctc(long_logits, lab, **kw)
    # the sheet functions on a synthetic sheet with a planted passage: a model whose logits are the planted ones
    labels = [4, 3, 9, 6]
    pred = _noisy(_planted([(4, 5, 10), (3, 15, 25), (11, 25, 32), (8, 32, 40), (9, 40, 45), (6, 50, 55)], 65, 14), 8)

    class Planted:
        """Stands in for the model: the sheet functions' align calls answered from the planted logits by the two-step route (its one
        body, which takes a confidence kind beside the pronunciation keywords as AlignModel.align does)."""

        def align(self, audios, labels, use_ctc=True, return_sheet_confidence=False, return_span_confidence=False,
                  return_anchored_confidence=False, **kw):
            kind = "sheet" if return_sheet_confidence else "anchored" if return_anchored_confidence else "span" if return_span_confidence else None
            return ua._perform(pred, labels, HOP, _lib.LA_VARIANT_CTC, 2, confidence=kind, **kw)

    syllables = ["sil"] + [f"s{i}" for i in range(1, 13)]
    lut = PinyinClassLUT(syllables, {s: i for i, s in enumerate(syllables)})
    lines, ids = ["一二", "三四"], {"一二": [4, 3], "三四": [9, 6]}
    old = align_record_lines(Planted(), None, lines, [False, False], lut, lambda t: ids[t])
    got, passages = align_record_lines(Planted(), None, lines, [False, False], lut, lambda t: ids[t], off_sheet=True)
    assert len(passages) == 1 and passages[0][0] == 1 and round(passages[0][1] / HOP) == 25 and round(passages[0][2] / HOP) == 40
    assert [[round(c[0] / HOP) for c in line] for line in got] == [[5, 15], [40, 50]] and got != old       # without the slots a character is stretched
    got2, passages2 = align_record_lines(Planted(), None, lines, [False, False], lut, lambda t: ids[t], off_sheet=[1])
    assert (got2, passages2) == (got, passages)
    (got3, pron3, passages3) = align_record_lines(Planted(), None, lines, [False, False], lut, lambda t: ids[t], off_sheet=True, with_pronunciation=True)
    assert got3 == got and passages3[0][:3] == passages[0] and passages3[0][3][0][0] in ("s11", "s8")
    (song, conf), passages4, prob = align_song(Planted(), None, lines, lut, lambda t: ids[t], off_sheet=True)
    assert song == got and passages4 == passages and sorted(prob) == [0, 1, 2] and prob[1] > 0.99 and prob[0] < 0.5 and "sung" in conf
    assert align_record_lines(Planted(), None, lines, [False, False], lut, lambda t: ids[t], off_sheet=False) == old
    # a confidence option adds {before_line: off_sheet_prob} as the last element, wherever pronunciation / heteronyms put theirs
    tok = lambda t: ids[t]
    (got5, sung), passages5, prob5 = align_record_lines(Planted(), None, lines, [False, False], lut, tok, off_sheet=True, with_confidence=True)
    assert got5 == got and passages5 == passages and sorted(prob5) == [0, 1, 2] and prob5[1] > 0.99 and prob5[0] < 0.5 and len(sung) == 2
    (got6, sung6), pron6, passages6, prob6 = align_record_lines(Planted(), None, lines, [False, False], lut, tok, off_sheet=True, with_confidence=True,
                                                                with_pronunciation=True)
    assert got6 == got and pron6 == pron3 and passages6 == passages3 and sorted(prob6) == [0, 1, 2] and prob6[1] > 0.99 and len(sung6) == 2
    ((song7, conf7), pron7, passages7, prob7) = align_song(Planted(), None, lines, lut, tok, off_sheet=True, with_pronunciation=True)
    assert song7 == got and pron7 == pron3 and passages7 == passages3 and sorted(prob7) == [0, 1, 2] and prob7[1] > 0.99 and "sung" in conf7
    (song8, conf8), passages8, prob8 = align_song(Planted(), None, lines, lut, tok, off_sheet=True, heteronyms={4: ["s5"]})
    assert [[c[:3] for c in line] for line in song8] == got and all(len(c) == 4 for line in song8 for c in line)
    assert passages8 == passages and sorted(prob8) == [0, 1, 2] and prob8[1] > 0.99
    # the LRC sheet: anchors and slots together, with and without the anchored confidence
    lrc = [(5 * HOP, lines[0]), (40 * HOP, lines[1])]
    got9, passages9 = align_record_lrc(Planted(), None, lrc, lut, tok, tolerance_s=3 * HOP, off_sheet=True)
    assert got9 == got and passages9 == passages
    (got10, conf10), passages10, prob10 = align_record_lrc(Planted(), None, lrc, lut, tok, tolerance_s=3 * HOP, off_sheet=True, with_confidence=True)
    assert got10 == got and passages10 == passages and sorted(prob10) == [0, 1, 2] and prob10[1] > 0.99 and "window_log_prob" in conf10
    with pytest.raises(ValueError, match="off_sheet"):
        align_record_lines(Planted(), None, lines, [False, False], lut, lambda t: ids[t], off_sheet=[3])
