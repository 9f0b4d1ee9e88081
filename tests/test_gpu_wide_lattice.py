"""Whole-song lattices on the device (la_viterbi_lattice_batch, ops.viterbi_lattice_batch and the layers over it): the span and window
faces of the strip kernel, 512 .. 4095 labels, bit for bit against the float64 restatement tests/windows_reference.py with rows=True
(pinned beyond 511 labels by tests/test_host_wide_lattice.py); against la_viterbi_batch with nothing given and with everything open;
few frames, one ragged launch, ties, the wrapper's refusals, then the Python surface on the tiny random-weight model."""
import functools

import numpy as np
import pytest
import torch

import windows_reference as wr
from test_gpu_windows import _assert_equals_reference, _emissions, _labels, _windows_around

pytestmark = pytest.mark.gpu

HOP = 0.02


def _sheet(seed, L):
    """skip_from of a random lyric sheet: lines of 1 .. 12 labels, about half of them optional.  One-label lines put a jump source among
    the target thread's own states; the last line, if optional, is a span that ends at n = L."""
    rs = np.random.RandomState(seed)
    skip = [-1] * (L + 1)
    pos = 0
    while pos < L:
        n = min(L, pos + int(rs.randint(1, 13)))
        if rs.rand() < 0.5:
            skip[n] = pos
        pos = n
    return skip


def _launch(ems, labels_list, skips, penalty, los=None, his=None):
    """Clips of different T / L in ONE la_viterbi_lattice_batch launch -> host arrays (onset, offset, score, status).  skips None: a null
    skip_from; los None: null windows.  Window rows are padded with the closed window [0, 0)."""
    from lyricalignment_amd import ops
    B = len(ems)
    Lmax = max(max(len(l) for l in labels_list), 1)
    Tmax = max(e.shape[0] for e in ems)
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
        if los is not None:
            lo[b, : len(los[b])] = torch.tensor(list(los[b]), dtype=torch.int32)
            hi[b, : len(his[b])] = torch.tensor(list(his[b]), dtype=torch.int32)
    n_labels = torch.tensor([len(l) for l in labels_list], dtype=torch.int32)
    n_frames = torch.tensor([e.shape[0] for e in ems], dtype=torch.int32)
    on, off, score, status = ops.viterbi_lattice_batch(em.cuda(), labels.cuda(), n_labels.cuda(), n_frames.cuda(),
                                                       None if skips is None else skip.cuda(), penalty,
                                                       None if los is None else lo.cuda(), None if los is None else hi.cuda())
    torch.cuda.synchronize()
    return on.cpu().numpy(), off.cpu().numpy(), score.cpu().numpy(), status.cpu().numpy()


def _n_left_out(ref, L):
    return sum(1 for n in range(L) if ref[0][n] < 0)


# ------------------------------------------------------------------------------------------------ 1. exact equality with the reference
SHAPES = [(560, 512),                     # 1025 states: the first strip size
          (700, 600),                     # R = 2
          (1300, 1100),                   # R = 4
          (2300, 2100),                   # R = 8
          (2600, 4095)]                   # the limit; more labels than frames, so only lattices with a sheet


@functools.lru_cache(maxsize=None)
def reference_cases(T, L):
    """The lattices of one shape with their yardstick results, computed once on the host (no GPU): per lattice a dict with the sheet, the
    penalty, the two clips' emissions, their windows, the windowed yardstick (refs) and the unwindowed one (free) of each clip.  Protocol of
    tests/test_gpu_windows.py test_equals_the_float64_reference_exactly: clip 0's windows lie around its own unwindowed best path, clip 1's
    around the unwindowed path of a SECOND emission draw, so that they bind."""
    lab = _labels(7 * T + L, L)
    S = 2 * L + 1
    sheet = _sheet(5 * T + L, L)
    assert any(a >= 0 and n - a == 1 for n, a in enumerate(sheet))          # a one-label optional line
    lattices = [(None, 0.0), (sheet, 0.0), (sheet, 1.0)]
    if L > T:
        lattices = lattices[1:]
    out = []
    for v, (skip, pen) in zip(range(3 - len(lattices), 3), lattices):
        rs = np.random.RandomState(1000 * v + 31 * T + L)
        ems = [_emissions(100 + v, T, lab, 0.0), _emissions(200 + v, T, lab, 1.5)]
        other = _emissions(300 + v, T, lab, 1.5 * (v % 2))
        refs, free, los, his = [], [], [], []
        for c, em in enumerate(ems):
            own = wr.viterbi_windows(em, lab, *wr.open_windows(L, T), skip, pen, rows=True)
            base = own if c == 0 else wr.viterbi_windows(other, lab, *wr.open_windows(L, T), skip, pen, rows=True)
            assert own[3] == wr.LA_OK and base[3] == wr.LA_OK, (T, L, v, c)
            lo, hi = _windows_around(rs, base[4], S, T)
            ref = wr.viterbi_windows(em, lab, lo, hi, skip, pen, rows=True)
            assert ref[3] == wr.LA_OK, (T, L, v, c)
            refs.append(ref); free.append(own); los.append(lo); his.append(hi)
        out.append(dict(v=v, skip=skip, pen=pen, lab=lab, ems=ems, refs=refs, free=free, los=los, his=his))
    return out


@pytest.mark.parametrize("T,L", SHAPES, ids=[f"T{t}_L{l}" for t, l in SHAPES])
def test_equals_the_float64_reference_exactly(T, L):
    """Per shape three lattices -- no spans (a null skip_from), a random sheet at penalty 0 and at penalty 1 -- each with two clips in one
    launch, on the window face; the same clips without windows on the span face (the plain strip kernel where there is no sheet).  Every
    case is LA_OK in the restatement, clip 1's windows change its result against the unwindowed restatement in every lattice, and every
    clip with a sheet leaves labels out; none is dropped."""
    cases = reference_cases(T, L)
    assert len(cases) == (2 if L > T else 3)
    for c in cases:
        v, skip, lab = c["v"], c["skip"], c["lab"]
        skips = None if skip is None else [skip, skip]
        got = _launch(c["ems"], [lab, lab], skips, c["pen"], c["los"], c["his"])
        for b in range(2):
            _assert_equals_reference(got, b, c["refs"][b], L, (T, L, v, b, "windows"))
        got = _launch(c["ems"], [lab, lab], skips, c["pen"])
        for b in range(2):
            _assert_equals_reference(got, b, c["free"][b], L, (T, L, v, b, "no windows"))
        # clip 0: the windows leave the best path in; clip 1: they bind
        assert c["refs"][0][:3] == c["free"][0][:3]
        assert c["refs"][1][0] != c["free"][1][0] or c["refs"][1][2] != c["free"][1][2], (T, L, v)
        if skip is not None:
            left = [_n_left_out(r, L) for r in c["refs"]]
            print(f"T={T} L={L} lattice {v}: labels left out {left}")
            assert min(left) > 0


# ------------------------------------------------------------------------------------------------ 2. few frames
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6, 9])
def test_few_frames_around_the_prefetch_depth(T):
    """512 labels in two optional halves, penalty 0.5, every window open: no path at T = 1, 2; from T = 3 on the path 0 -> 512 -> 1024 that
    leaves every label out."""
    L = 512
    lab = _labels(3, L)
    skip = [-1] * (L + 1)
    skip[256], skip[512] = 0, 256
    em = _emissions(40 + T, T, lab, 0.0)
    lo, hi = wr.open_windows(L, T)
    ref = wr.viterbi_windows(em, lab, lo, hi, skip, 0.5, rows=True)
    assert ref[3] == (wr.LA_EINFEASIBLE if T <= 2 else wr.LA_OK)
    if T >= 3:
        assert ref[0] == [-1] * L and ref[4][0] == 0 and ref[4][-1] == 2 * L and 2 * 256 in ref[4]
    _assert_equals_reference(_launch([em], [lab], [skip], 0.5, [lo], [hi]), 0, ref, L, ("windows", T))
    _assert_equals_reference(_launch([em], [lab], [skip], 0.5), 0, ref, L, ("no windows", T))


@pytest.mark.parametrize("L", [512, 1024, 2048])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6, 9])
def test_plain_strip_loop_at_few_frames(T, L):
    """The span-free frame loop of the strip kernel (the plain DP's loop for every song over 511 labels) at the first label counts of 2, 4
    and 8 states per thread, T around the prefetch depth of 4 and two blocks plus one, through la_viterbi_batch and through
    la_viterbi_lattice_batch with nothing given.  L > T: no such lattice has a path, so this pins the tie rules on rows of equal kNeg cells
    and the tail of a partial prefetch block."""
    from lyricalignment_amd import ops
    lab = [int(v) for v in np.random.RandomState(11 * T + L).randint(1, 4, size=L)]     # three classes: equal neighbours everywhere
    em = _emissions(60 + T, T, lab, 0.0)
    ref = wr.viterbi_windows(em, lab, *wr.open_windows(L, T), None, 0.0, rows=True)
    assert ref[3] == wr.LA_EINFEASIBLE
    _assert_equals_reference(_launch([em], [lab], None, 0.0), 0, ref, L, ("lattice, nothing given", T, L))
    got = ops.viterbi_batch(torch.from_numpy(em)[None].cuda(), torch.tensor([lab], dtype=torch.int32).cuda(),
                            torch.tensor([L], dtype=torch.int32).cuda(), torch.tensor([T], dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    _assert_equals_reference(tuple(g.cpu().numpy() for g in got), 0, ref, L, ("viterbi_batch", T, L))


# ------------------------------------------------------------------------------------------------ 3. nothing given and all open
def _dev_inputs(ems, lab):
    B, T, L = len(ems), ems[0].shape[0], len(lab)
    em = torch.from_numpy(np.ascontiguousarray(np.stack(ems))).cuda()
    labels = torch.tensor([lab] * B, dtype=torch.int32).cuda()
    return em, labels, torch.full((B,), L, dtype=torch.int32).cuda(), torch.full((B,), T, dtype=torch.int32).cuda()


def _assert_same(want, got, what):
    for name, w, g in zip(("onset", "offset", "score", "status"), want, got):
        assert torch.equal(w, g), (what, name)
    assert want[2].cpu().numpy().tobytes() == got[2].cpu().numpy().tobytes(), what


@pytest.mark.parametrize("T,L", [(700, 600), (2300, 2100), (300, 100), (90, 31)])
def test_nothing_given_and_all_open_equal_the_existing_entries_bit_for_bit(T, L):
    from lyricalignment_amd import ops
    lab = _labels(5, L)
    em, labels, n_lab, n_fr = _dev_inputs([_emissions(1, T, lab, 0.0), _emissions(2, T, lab, 1.5)], lab)
    none = torch.full((2, L + 1), -1, dtype=torch.int32).cuda()
    lo = torch.zeros((2, 2 * L + 1), dtype=torch.int32).cuda()
    hi = torch.full((2, 2 * L + 1), T, dtype=torch.int32).cuda()
    plain = ops.viterbi_batch(em, labels, n_lab, n_fr)
    assert (plain[3] == 0).all()
    _assert_same(plain, ops.viterbi_lattice_batch(em, labels, n_lab, n_fr), "nothing given")
    _assert_same(plain, ops.viterbi_lattice_batch(em, labels, n_lab, n_fr, none, 0.75), "an all -1 skip_from")
    _assert_same(plain, ops.viterbi_lattice_batch(em, labels, n_lab, n_fr, None, 0.0, lo, hi), "open windows")
    _assert_same(plain, ops.viterbi_lattice_batch(em, labels, n_lab, n_fr, none, 0.75, lo, hi), "open windows, an all -1 skip_from")
    if L <= 511:            # the call IS the matching entry's
        skip = torch.tensor([_sheet(9, L)] * 2, dtype=torch.int32).cuda()
        spans = ops.viterbi_spans_batch(em, labels, n_lab, n_fr, skip, 0.25)
        assert int((spans[0] < 0).sum()) > 0
        _assert_same(spans, ops.viterbi_lattice_batch(em, labels, n_lab, n_fr, skip, 0.25), "spans")
        hi2 = hi - 7
        for s in (None, skip):
            _assert_same(ops.viterbi_windows_batch(em, labels, n_lab, n_fr, lo, hi2, s, 0.25),
                         ops.viterbi_lattice_batch(em, labels, n_lab, n_fr, s, 0.25, lo, hi2), ("windows", s is not None))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. one ragged launch
def test_ragged_launch_each_clip_equals_the_reference_alone():
    """A whole song with sheet and windows, a small lattice inside the strip launch, a clip too short for its labels, a clip without labels,
    a clip with windows around its best path of which one mandatory label's is closed (no path: -inf), and a clip with a sheet only, in
    one launch."""
    rs = np.random.RandomState(4)
    shapes = [(1800, 700), (900, 30), (650, 640), (1300, 0), (2000, 513), (1290, 640)]
    labs = [_labels(10 + i, L) if L else [] for i, (_, L) in enumerate(shapes)]
    ems = [_emissions(20 + i, T, lab, 1.5 if i in (0, 5) else 0.0) if lab else np.zeros((T, 1), np.float32)
           for i, ((T, _), lab) in enumerate(zip(shapes, labs))]
    skips = [_sheet(30 + i, L) if i in (0, 5) else [-1] * (L + 1) for i, (_, L) in enumerate(shapes)]
    los, his = [], []
    for i, (T, L) in enumerate(shapes):
        lo, hi = wr.open_windows(L, T)
        if i in (0, 4):                      # windows around a path of the lattice: of a second emission draw (clip 0), its own (clip 4)
            path = wr.viterbi_windows(_emissions(40, T, labs[i], 0.0) if i == 0 else ems[i], labs[i], lo, hi, skips[i], 0.5, rows=True)[4]
            lo, hi = _windows_around(rs, path, 2 * L + 1, T)
        if i == 4:
            lo[2 * 200 + 1] = hi[2 * 200 + 1] = 1000               # label 200 (mandatory: this clip has no span) is never allowed
        los.append(lo); his.append(hi)
    refs = [wr.viterbi_windows(em, lab, lo, hi, skip, 0.5, rows=True) for em, lab, lo, hi, skip in zip(ems, labs, los, his, skips)]
    assert [r[3] for r in refs] == [wr.LA_OK, wr.LA_OK, wr.LA_EINFEASIBLE, wr.LA_EEMPTY, wr.LA_EINFEASIBLE, wr.LA_OK]
    assert refs[4][2] == -np.inf and refs[2][2] > -np.inf
    assert _n_left_out(refs[0], 700) > 0 and _n_left_out(refs[5], 640) > 0
    got = _launch(ems, labs, skips, 0.5, los, his)
    on, off, score, status = got
    for b, (T, L) in enumerate(shapes):
        if L:
            _assert_equals_reference(got, b, refs[b], L, b)
    assert status[3] == wr.LA_EEMPTY and (on[3] == -1).all() and (off[3] == -1).all()
    assert score[4] == -np.inf and (on[4] == -1).all() and (off[4] == -1).all()


# ------------------------------------------------------------------------------------------------ 5. ties
@pytest.mark.parametrize("pen", [0.0, 1.0])
def test_ties_are_broken_in_the_reference_order(pen):
    """Every emission 0.0: the result is pure comparison order (strictly greater, J before J-1), with and without (open) windows."""
    T, L = 700, 600
    lab = _labels(7 * T + L, L)
    skip = _sheet(5 * T + L, L)
    em = np.zeros((T, L + 1), np.float32)
    lo, hi = wr.open_windows(L, T)
    ref = wr.viterbi_windows(em, lab, lo, hi, skip, pen, rows=True)
    assert ref[3] == wr.LA_OK
    _assert_equals_reference(_launch([em], [lab], [skip], pen, [lo], [hi]), 0, ref, L, "windows")
    _assert_equals_reference(_launch([em], [lab], [skip], pen), 0, ref, L, "no windows")


# ------------------------------------------------------------------------------------------------ 6. the wrapper
def test_ops_wrapper_rejects_bad_arguments():
    from lyricalignment_amd import ops
    em = torch.zeros((2, 10, 5), dtype=torch.float32).cuda()
    lab = torch.ones((2, 4), dtype=torch.int32).cuda()
    n = torch.tensor([4, 4], dtype=torch.int32).cuda()
    t = torch.tensor([10, 10], dtype=torch.int32).cuda()
    lo = torch.zeros((2, 9), dtype=torch.int32).cuda()
    hi = torch.full((2, 9), 10, dtype=torch.int32).cuda()
    skip = torch.full((2, 5), -1, dtype=torch.int32).cuda()
    assert ops.viterbi_lattice_batch(em, lab, n, t, skip, 0.0, lo, hi)[3].tolist() == [0, 0]
    for bad in ((lo[:, :8], hi), (lo, hi[:, :8].contiguous()), (lo.long(), hi), (lo.cpu(), hi), (lo[:1], hi), (lo, None), (None, hi)):
        with pytest.raises(ValueError):
            ops.viterbi_lattice_batch(em, lab, n, t, None, 0.0, *bad)
    with pytest.raises(ValueError):
        ops.viterbi_lattice_batch(em, lab, n, t, skip[:, :4], 0.0, lo, hi)
    with pytest.raises(ValueError):
        ops.viterbi_lattice_batch(em, lab, n, t, skip, -1.0, lo, hi)
    with pytest.raises(ValueError):
        ops.viterbi_lattice_batch(em, lab, n, t, None, float("nan"), lo, hi)
    wide = (torch.zeros((1, 4, 4097), dtype=torch.float32).cuda(), torch.ones((1, 4096), dtype=torch.int32).cuda(), n[:1], t[:1])
    with pytest.raises(NotImplementedError, match="4095"):
        ops.viterbi_lattice_batch(*wide, torch.full((1, 4097), -1, dtype=torch.int32).cuda())
    with pytest.raises(NotImplementedError, match="511"):
        ops.viterbi_spans_batch(torch.zeros((1, 4, 513), dtype=torch.float32).cuda(), torch.ones((1, 512), dtype=torch.int32).cuda(),
                                n[:1], t[:1], torch.full((1, 513), -1, dtype=torch.int32).cuda())


# ------------------------------------------------------------------------------------------------ 7. the Python surface on the tiny model
@pytest.fixture(scope="module")
def tiny():
    import test_gpu_ragged as tr
    from test_gpu_parity_full import _build
    model, _ = _build("tiny", torch.float32)
    return dict(model=model, tr=tr)


def test_a_whole_sheet_of_600_labels_through_align_and_align_record_lrc(tiny):
    """A 33 s recording (1650 frames) against 600 labels in lines of 10, every third line optional, one onset anchor per line at the onset
    the sheet-only alignment gave the line's first character (or the next sung line's), tolerance 1 s."""
    from lyricalignment_amd import _lib, ops
    from lyricalignment_amd.harness import PinyinClassLUT, align_record_lines, align_record_lrc
    from lyricalignment_amd.utils import alignment as ua
    from test_gpu_parity_full import VOCAB
    model, tr = tiny["model"], tiny["tr"]
    audio = np.concatenate([tr._clip(4), tr._clip(3)])
    L, n_lines = 600, 60
    ids_all = [int(v) for v in np.random.RandomState(6).randint(2, 403, size=L)]
    labels = torch.tensor([ids_all], dtype=torch.long)
    optional = [i % 3 == 2 for i in range(n_lines)]
    spans = [(10 * i, 10 * i + 10) for i in range(n_lines) if optional[i]]
    with torch.no_grad():
        logits, _ = model.frame_manual_forward([audio])
        T = logits.shape[1]
        assert T == 1650
        sheet_only = model.align([audio], labels, optional_spans=[spans], return_frames=True)
        assert sheet_only[3].tolist() == [0]
        on = sheet_only[0][0].tolist()
        starts, nxt = [0.0] * n_lines, float(T - 1) * HOP
        for i in range(n_lines - 1, -1, -1):                      # a line left out takes the next sung line's onset
            if on[10 * i] >= 0:
                nxt = float(on[10 * i]) * HOP
            starts[i] = nxt
        anchors = [(10 * i, starts[i], 1.0) for i in range(n_lines)]
        kw = dict(optional_spans=[spans], onset_anchors=[anchors], skip_penalty=0.5)
        fused = model.align([audio], labels, **kw)
        assert fused == ua.perform_viterbi_ctc(logits, labels, **kw)
        frames = model.align([audio], labels, return_frames=True, **kw)
        assert frames[3].tolist() == [0]
        # the yardstick on the emissions the two-step route computes
        lab_dev, n_lab, lists = ua._labels_to_device(labels, 1, logits.device)
        em = ops.emissions_from_logits(logits.float().contiguous(), lab_dev, n_lab, _lib.LA_VARIANT_CTC)
        lo, hi = ua._windows_of(None, [anchors], lists, [T], HOP)
        skip = ua._skip_from_of_spans([spans], lists)
        ref = wr.viterbi_windows(em[0].cpu().numpy(), lists[0], lo[0].tolist(), hi[0].tolist(), skip[0].tolist(), 0.5, rows=True)
        assert ref[3] == wr.LA_OK
        assert frames[0][0].tolist() == ref[0] and frames[1][0].tolist() == ref[1]
        # the sheet functions: one entry per line, None or one triple per character
        lut = PinyinClassLUT([str(i) for i in range(VOCAB)], {str(i): i for i in range(VOCAB)})
        lines = ["".join(chr(0x4E00 + 10 * k + j) for j in range(10)) for k in range(n_lines)]
        ids = {line: ids_all[10 * k: 10 * k + 10] for k, line in enumerate(lines)}
        got = align_record_lrc(model, audio, list(zip(starts, lines)), lut, lambda t: ids[t], tolerance_s=1.0, optional=optional, skip_penalty=0.5)
        assert len(got) == n_lines
        for i, (entry, line) in enumerate(zip(got, lines)):
            part = fused[0][10 * i: 10 * i + 10]
            if entry is None:
                assert optional[i] and all(c is None for c in part)
            else:
                assert entry == [[c[0], c[1], ch] for c, ch in zip(part, line)]
        by_lines = align_record_lines(model, audio, lines, optional, lut, lambda t: ids[t])
        assert [e is None for e in by_lines] == [v < 0 for v in on[::10]]
        # the posterior sweeps stop at 511 labels
        with pytest.raises(NotImplementedError, match="511"):
            model.align([audio], labels, return_anchored_confidence=True, **kw)
        with pytest.raises(NotImplementedError, match="511"):
            model.align([audio], labels, optional_spans=[spans], return_span_confidence=True)
        with pytest.raises(NotImplementedError, match="511"):
            align_record_lrc(model, audio, list(zip(starts, lines)), lut, lambda t: ids[t], optional=optional, with_confidence=True)
        with pytest.raises(NotImplementedError, match="511"):
            align_record_lines(model, audio, lines, optional, lut, lambda t: ids[t], with_confidence=True)
