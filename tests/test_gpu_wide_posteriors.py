"""Whole-song posteriors on the device (la_alignment_posteriors_lattice: posterior_strip_kernel of csrc/la_posterior.hip beyond 511
labels, the lane-per-state posterior_kernel of the same file below) and the layers over it (ops.alignment_posteriors_lattice,
run_lattice(confidence="sheet"), AlignModel.align(return_sheet_confidence=True), perform_viterbi(_ctc)_sheet_scored, harness.align_song).

Yardstick: window_posterior_reference.posteriors plus span_posterior_reference.scores on the onset / offset of
windows_reference.viterbi_windows(..., rows=True) -- float64, pinned to path enumeration by the host tests of those modules.

Tolerance: absolute 8 * T * 2**-23 on gamma (every cell), the five per-label outputs and log_z, derived in tests/test_gpu_span_posteriors.py;
16 * T * 2**-23 on window_log_prob, a difference of two log_z.  It carries over to the strip kernel because every cell is computed by the
expression sequence of the lane-per-state kernel (test A3 holds bit for bit) and a closed or absent cell adds no rounding.  No cell, label
or clip is exempt.  Every test prints its measured maxima before it asserts (on record: 3.2e-6 on gamma and the per-label outputs,
7.4e-6 on log_z up to 2048 labels, 9.6e-6 at 4095; DESIGN.md "Whole-song posteriors").

A thread's first state k0 = tid * R is even, so a label's state is never the first state of a thread; the equal-neighbour pair of the
case list sits where the second label's state is the first label state of its thread instead (wide_posterior_cases.labels_of)."""
import json

import numpy as np
import pytest
import torch

import span_posterior_reference as spr
import wide_posterior_cases as wpc
import window_posterior_reference as wpr
import windows_reference as wr
from test_gpu_window_posteriors import NAMES, PROBS, SHARED, _assert_no_path, _compare, _tol
from test_gpu_windows import _emissions, _labels, _two_optional_lines

pytestmark = pytest.mark.gpu

HOP = 0.02
OUT = NAMES + ("gamma",)


def _launch(ems, labs, skips, pen, los, his, ons, offs, Tmax=None, Lmax=None, T_list=None, gamma=True, op=None):
    """Clips of different T / L in ONE ops.alignment_posteriors_lattice launch (or one launch of `op`, an existing entry's wrapper with the
    same lattice) -> dict of host arrays.  skips None: a null skip_from; los None: null windows.  Window rows are padded with the closed
    window [0, 0), onset / offset rows with -1."""
    from lyricalignment_amd import ops
    B = len(ems)
    Lmax = Lmax or max(max(len(l) for l in labs), 1)
    Tmax = Tmax or max(e.shape[0] for e in ems)
    em = torch.zeros((B, Tmax, Lmax + 1), dtype=torch.float32)
    labels = torch.zeros((B, Lmax), dtype=torch.int32)
    skip = torch.full((B, Lmax + 1), -1, dtype=torch.int32)
    lo = torch.zeros((B, 2 * Lmax + 1), dtype=torch.int32)
    hi = torch.zeros((B, 2 * Lmax + 1), dtype=torch.int32)
    on = torch.full((B, Lmax), -1, dtype=torch.int32)
    off = torch.full((B, Lmax), -1, dtype=torch.int32)
    for b, (e, l) in enumerate(zip(ems, labs)):
        em[b, : e.shape[0], : e.shape[1]] = torch.from_numpy(np.array(e))       # (a copy: the shared cases are read-only)
        labels[b, : len(l)] = torch.tensor(list(l), dtype=torch.int32)
        if skips is not None:
            skip[b, : len(skips[b])] = torch.tensor(list(skips[b]), dtype=torch.int32)
        if los is not None:
            lo[b, : len(los[b])] = torch.tensor(list(los[b]), dtype=torch.int32)
            hi[b, : len(his[b])] = torch.tensor(list(his[b]), dtype=torch.int32)
        on[b, : len(l)] = torch.tensor(list(ons[b])[: len(l)], dtype=torch.int32)
        off[b, : len(l)] = torch.tensor(list(offs[b])[: len(l)], dtype=torch.int32)
    n_labels = torch.tensor([len(l) for l in labs], dtype=torch.int32)
    n_frames = torch.tensor([e.shape[0] for e in ems] if T_list is None else T_list, dtype=torch.int32)
    dev = [t.cuda() for t in (em, labels, n_labels, n_frames, on, off)]
    sk = None if skips is None else skip.cuda()
    win = (None, None) if los is None else (lo.cuda(), hi.cuda())
    if op is None:
        res = ops.alignment_posteriors_lattice(*dev, sk, pen, *win, boundary_window=2, want_gamma=gamma)
    elif op == "windows":
        res = ops.alignment_posteriors_windows(*dev, *win, sk, pen, boundary_window=2, want_gamma=gamma)
    elif op == "spans":
        res = ops.alignment_posteriors_spans(*dev, sk, pen, boundary_window=2, want_gamma=gamma)
    else:
        res = ops.alignment_posteriors(*dev, boundary_window=2, want_gamma=gamma)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in zip((SHARED if op == "plain" else NAMES) + (("gamma",) if gamma else ()), res)}
    out.update(onset=on.numpy(), offset=off.numpy())
    return out


def _same_bytes(a, b, what, keys=OUT):
    for key in keys:
        assert a[key].tobytes() == b[key].tobytes(), (what, key)


def _report(what, T, total):
    print(f"{what}: tol={_tol(T):.2e}, measured maxima: " + json.dumps({k: float(f"{v:.2e}") for k, v in total.items()}))


# ------------------------------------------------------------------------------------------------ A1. every output against the yardstick
@pytest.mark.parametrize("v", range(4), ids=[n.replace(" ", "_").replace(",", "") for n in wpc.LATTICES])
@pytest.mark.parametrize("T,L", wpc.SHAPES, ids=[f"T{t}_L{l}" for t, l in wpc.SHAPES])
def test_shapes_match_the_yardstick_in_every_output_and_every_gamma_cell(T, L, v):
    from lyricalignment_amd import _lib
    c = wpc.lattice_case(T, L, v)
    skip, lab, em = c["skip"], c["lab"], c["em"]
    if skip is not None:                    # what the span set has to hold
        spans = spr.spans_of(skip)
        assert any(n - a == 1 for a, n in spans) and any(a == 0 for a, n in spans) and any(n == L for a, n in spans)
        assert any(n - a > 256 for a, n in spans) and len({a for a, n in spans}) < len(spans)
        assert any(a1 < a2 and n2 < n1 for a1, n1 in spans for a2, n2 in spans)
        # a thread folds more arc words than the four it holds in registers, beside shorter lists in its wave
        print(f"T={T} L={L} arc lists above four words in one wave: {wpc.assert_long_arc_lists(skip, lab, wpc.strip_states_per_thread(L))}")
    assert lab[64] == lab[63] and (2 * 64 + 1) % 8 == 1
    r = _launch([em], [lab], None if skip is None else [skip], c["pen"], None if c["lo"] is None else [c["lo"]],
                None if c["hi"] is None else [c["hi"]], [c["on"]], [c["off"]])
    assert r["status"][0] == _lib.LA_OK
    r["score"] = np.array([c["score"]])
    lo, hi = (c["lo"], c["hi"]) if c["lo"] is not None else wr.open_windows(L, T)
    worst = _compare(r, 0, c["ref"], em, lab, skip, lo, hi, 2)
    _report(f"T={T} L={L} {c['name']}", T, worst)
    if skip is not None:
        assert (r["span_skip_prob"][0] > 1e-3).sum() > 0                  # jumps carry mass
    else:
        assert (r["present_prob"][0, :L] == 1.0).all() and not r["span_skip_prob"].any()
    bad = {k: float(x) for k, x in worst.items() if not x <= _tol(T)}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ A2. T below L
def test_fewer_frames_than_labels():
    """(400, 600): with every line optional the lattice has paths only through jumps; without spans, and with windows that close both start
    states, it has none."""
    from lyricalignment_amd import _lib
    T, L = 400, 600
    lab = _labels(17, L)
    em = _emissions(18, T, lab, 1.0)
    skip = wpc.every_line_optional(L)
    y = wpc.yardstick(em, lab, skip, 0.5)
    assert y["status"] == wr.LA_OK and np.isfinite(y["ref"][5]) and sum(1 for n in y["on"] if n < 0) >= L - T
    r = _launch([em], [lab], [skip], 0.5, None, None, [y["on"]], [y["off"]])
    assert r["status"][0] == _lib.LA_OK
    r["score"] = np.array([y["score"]])
    worst = _compare(r, 0, y["ref"], em, lab, skip, *wr.open_windows(L, T), 2)
    _report("T=400 L=600 every line optional", T, worst)
    assert all(x <= _tol(T) for x in worst.values()), worst
    none = [-1] * L
    _assert_no_path(_launch([em], [lab], None, 0.5, None, None, [none], [none]), 0, "no spans")
    _assert_no_path(_launch([em], [lab], [[-1] * (L + 1)], 0.5, None, None, [none], [none]), 0, "an all -1 skip_from")
    lo, hi = wr.open_windows(L, T)
    lo[0] = lo[1] = 1
    assert np.isneginf(wpr.posteriors(em, lab, lo, hi, skip, 0.5)[5])
    _assert_no_path(_launch([em], [lab], [skip], 0.5, [lo], [hi], [none], [none]), 0, "both start states closed")


# ------------------------------------------------------------------------------------------------ A2b. a few frames
@pytest.mark.parametrize("T", [1, 2, 3, 6, 7])
@pytest.mark.parametrize("L", [512, 1100, 2100])
def test_a_few_frames_on_the_strip_kernel(T, L):
    """Where the cell's t == T-1 and t > 0 branches and the tail of the prefetch blocks (4, 2 and 1 frames at 2, 4 and 8 states per thread)
    meet.  Every line optional, plus spans from label 0 to L-3 and to L; the emissions plant the last three labels at frames 1, 3 and 5.
    One frame: no path.  Two or three: every label skipped.  Six or seven: exactly the last three labels sung, so all three sums run."""
    lab = wpc.labels_of(3, L)
    em = (-3 - np.random.RandomState(T + L).rand(T, L + 1) * 3).astype(np.float32)
    for i, n in enumerate((L - 3, L - 2, L - 1)):
        if 1 + 2 * i < T:
            em[1 + 2 * i, 1 + n] = -0.1
    skip = wpc.every_line_optional(L)
    skip[L] = skip[L - 3] = 0
    y = wpc.yardstick(em, lab, skip, 0.5)
    assert y["status"] == (wr.LA_EINFEASIBLE if T == 1 else wr.LA_OK) and np.isneginf(y["ref"][5]) == (T == 1)
    if T > 1:
        sung = [n for n in range(L) if y["on"][n] >= 0]
        assert sung == ([L - 3, L - 2, L - 1] if T >= 6 else []), sung
    r = _launch([em], [lab], [skip], 0.5, None, None, [y["on"]], [y["off"]])
    if T == 1:
        _assert_no_path(r, 0, "one frame")
        return
    from lyricalignment_amd import _lib
    assert r["status"][0] == _lib.LA_OK
    r["score"] = np.array([y["score"]])
    worst = _compare(r, 0, y["ref"], em, lab, skip, *wr.open_windows(L, T), 2)
    _report(f"T={T} L={L} a few frames", T, worst)
    assert all(x <= _tol(T) for x in worst.values()), worst


# ------------------------------------------------------------------------------------------------ A3. mixed batch, bit equality
@pytest.mark.parametrize("face", ["windows", "spans"])
def test_mixed_batch_equals_the_lane_per_state_kernel_bit_for_bit(face):
    """One launch with max_labels = 600: clips of 5, 300, 511 and 600 labels with different frame counts and a clip too short for its
    labels.  The strip kernel runs all of them; the three small ones equal the lane-per-state kernel's run of that clip alone in every
    output byte and gamma cell, every clip equals itself run alone through the new entry, and a second call repeats the first.  The
    511-label clip carries wide_posterior_cases.long_arc_lists beside its two optional lines, so the strip kernel folds arc lists longer
    than its four register words (two states per thread here) against the lane-per-state kernel's fold."""
    from lyricalignment_amd import _lib
    shapes = [(40, 5), (400, 300), (600, 511), (700, 600), (200, 300)]
    labs = [_labels(20 + i, L) for i, (_, L) in enumerate(shapes)]
    ems = [_emissions(30 + i, T, lab, 1.0) for i, ((T, _), lab) in enumerate(zip(shapes, labs))]
    skips = [_two_optional_lines(5), _two_optional_lines(300), wpc.long_arc_lists(_two_optional_lines(511)), wpc.span_set(600), [-1] * 301]
    for b in (2, 3):
        print(f"clip {b}: arc lists above four words in one wave: {wpc.assert_long_arc_lists(skips[b], labs[b], wpc.strip_states_per_thread(600))}")
    los = his = None
    if face == "windows":
        los, his = [], []
        for i, (T, L) in enumerate(shapes):
            lo, hi = wpc.narrowed_windows(ems[i], labs[i], skips[i], 0.5) if i < 4 else wr.open_windows(L, T)
            los.append(lo); his.append(hi)
    dps = [wr.viterbi_windows(em, lab, *(wr.open_windows(len(lab), em.shape[0]) if los is None else (los[i], his[i])), skips[i], 0.5, rows=True)
           for i, (em, lab) in enumerate(zip(ems, labs))]
    assert [d[3] for d in dps] == [wr.LA_OK] * 4 + [wr.LA_EINFEASIBLE]
    ons, offs = [d[0] for d in dps], [d[1] for d in dps]
    r = _launch(ems, labs, skips, 0.5, los, his, ons, offs)
    assert r["status"].tolist() == [_lib.LA_OK] * 4 + [_lib.LA_EINFEASIBLE]
    _assert_no_path(r, 4, "too short")
    _same_bytes(r, _launch(ems, labs, skips, 0.5, los, his, ons, offs), "a second call")
    for b, (T, L) in enumerate(shapes):
        S = 2 * L + 1
        one = lambda x: None if x is None else [x[b]]
        alone = _launch([ems[b]], [labs[b]], [skips[b]], 0.5, one(los), one(his), [ons[b]], [offs[b]])
        lane = _launch([ems[b]], [labs[b]], [skips[b]], 0.5, one(los), one(his), [ons[b]], [offs[b]], op=face) if L <= 511 else None
        for other, what in ((alone, "alone through the new entry"), (lane, "the lane-per-state kernel alone")):
            if other is None:
                continue
            for key in PROBS:
                n = L + (key == "span_skip_prob")
                assert r[key][b, :n].tobytes() == other[key][0, :n].tobytes(), (b, what, key)
                assert not r[key][b, n:].any()
            assert r["log_z"][b].tobytes() == other["log_z"][0].tobytes() and r["status"][b] == other["status"][0], (b, what)
            assert np.ascontiguousarray(r["gamma"][b, :T, :S]).tobytes() == other["gamma"][0].tobytes(), (b, what, "gamma")
        assert not r["gamma"][b, T:].any() and not r["gamma"][b, :, S:].any()
    assert (r["span_skip_prob"] > 1e-3).sum() > 0
    with pytest.raises(NotImplementedError, match="511"):                                  # the existing entries keep their limit
        _launch([ems[3]], [labs[3]], [skips[3]], 0.5, [wr.open_windows(600, 700)[0]], [wr.open_windows(600, 700)[1]], [ons[3]], [offs[3]], op=face)


# ------------------------------------------------------------------------------------------------ A4. up to 511 labels
@pytest.mark.parametrize("T,L,dpp", [(300, 100, 1), (600, 511, 1), (90, 31, 1), (90, 31, 0)])
def test_up_to_511_labels_the_new_entry_is_the_matching_existing_entry(T, L, dpp):
    """Three clips in one launch -- all L labels, half of them, and all of them in three frames (no path) -- through the new entry with
    windows (with and without a skip_from), with spans only and with nothing given, against la_alignment_posteriors_windows / _spans /
    la_alignment_posteriors: the same bytes.  With nothing given present_prob is 1 on the labels of an LA_OK clip and 0 elsewhere,
    span_skip_prob 0: what the spans entry gives for an all -1 skip_from."""
    from lyricalignment_amd import _lib
    lab = _labels(5, L)
    labs = [lab, lab[: L // 2], lab]
    ems = [_emissions(1, T, lab, 2.0), _emissions(2, T, labs[1], 2.0), _emissions(3, 3, lab, 0.0)]     # leaving a line out pays
    skips = [_two_optional_lines(len(l)) for l in labs[:2]] + [[-1] * (L + 1)]
    none = [[-1] * (len(l) + 1) for l in labs]

    def narrowed(sk):                           # two states of each clip's own path narrowed; the clip without a path keeps open windows
        wins = [wpc.narrowed_windows(ems[b], labs[b], sk[b], 0.5) for b in range(2)] + [wr.open_windows(L, 3)]
        return [w[0] for w in wins], [w[1] for w in wins]
    with _lib.option("viterbi_dpp", dpp):
        for sk, (lo, hi), op in ((skips, narrowed(skips), "windows"), (None, narrowed(none), "windows"), (skips, (None, None), "spans"),
                                 (None, (None, None), "plain")):
            dps = [wr.viterbi_windows(ems[b], labs[b], *(wr.open_windows(len(labs[b]), ems[b].shape[0]) if lo is None else (lo[b], hi[b])),
                                      (sk or none)[b], 0.5, rows=True) for b in range(3)]
            assert [d[3] for d in dps] == [wr.LA_OK, wr.LA_OK, wr.LA_EINFEASIBLE]
            ons, offs = [d[0] for d in dps], [d[1] for d in dps]
            new = _launch(ems, labs, sk, 0.5, lo, hi, ons, offs)
            old = _launch(ems, labs, sk, 0.5, lo, hi, ons, offs, op=op)
            assert new["status"].tolist() == [0, 0, _lib.LA_EINFEASIBLE]
            _same_bytes(new, old, (op, sk is not None), SHARED + ("gamma",) if op == "plain" else OUT)
            if op == "plain":
                all_minus_one = _launch(ems, labs, none, 0.5, None, None, ons, offs, op="spans")
                _same_bytes(new, all_minus_one, "an all -1 skip_from through the spans entry")
                want = np.zeros((3, L), np.float32)
                want[0, :L] = 1.0
                want[1, : L // 2] = 1.0
                assert (new["present_prob"] == want).all() and not new["span_skip_prob"].any()
            elif sk is not None:
                assert new["span_skip_prob"][:2].max() > 1e-3                          # jumps carry mass


# ------------------------------------------------------------------------------------------------ A5. open windows
@pytest.mark.parametrize("v", [0, 2], ids=["no_spans", "spans"])
def test_every_window_open_equals_no_windows_given_bit_for_bit(v):
    T, L = 1100, 1024
    c = wpc.lattice_case(T, L, v)
    lo, hi = wr.open_windows(L, T)
    skips = None if c["skip"] is None else [c["skip"]]
    a = _launch([c["em"]], [c["lab"]], skips, c["pen"], [lo], [hi], [c["on"]], [c["off"]])
    b = _launch([c["em"]], [c["lab"]], skips, c["pen"], None, None, [c["on"]], [c["off"]])
    assert a["status"][0] == 0 and a["gamma"].any()
    _same_bytes(a, b, c["name"])


# ------------------------------------------------------------------------------------------------ A6. the top of the range
def test_4095_labels_and_the_refusal_at_4096():
    """(4200, 4095) with the span set: LA_OK, log_z within the bound of a forward-only float64 numpy sweep, the coverage identity and the
    row sums of gamma on the device's output.  The full yardstick would take 14 s and 2.7 GB here."""
    from lyricalignment_amd import _lib, ops
    T, L = 4200, 4095
    lab = wpc.labels_of(3, L)
    em = _emissions(4, T, lab, 1.0)
    skip = wpc.span_set(L)
    dev = (torch.from_numpy(em)[None].cuda(), torch.tensor([lab], dtype=torch.int32).cuda(), torch.tensor([L], dtype=torch.int32).cuda(),
           torch.tensor([T], dtype=torch.int32).cuda())
    sk = torch.tensor([skip], dtype=torch.int32).cuda()
    on, off, score, status = ops.viterbi_lattice_batch(*dev, sk, 0.5)
    assert status.tolist() == [_lib.LA_OK]
    res = ops.alignment_posteriors_lattice(*dev, on, off, sk, 0.5, want_gamma=True)
    torch.cuda.synchronize()
    assert res[4].tolist() == [_lib.LA_OK]
    rowsum = res[7][0].double().sum(1).cpu().numpy()
    gmin, gmax = float(res[7].min()), float(res[7].max())
    present, span_skip = res[5][0].cpu().numpy().astype(np.float64), res[6][0].cpu().numpy().astype(np.float64)
    want = wpc.forward_log_z(em, lab, skip, 0.5)
    worst = {"log_z": abs(float(res[3][0]) - want), "gamma_rowsum": np.abs(rowsum - 1).max(), "gamma_range": max(0.0, -gmin, gmax - 1),
             "coverage": np.abs(spr.coverage(present, span_skip, skip) - 1).max(), "path_above_total": max(0.0, float(score[0] - res[3][0]))}
    for key, val in zip(PROBS, res[:3] + res[5:7]):
        val = val.cpu().numpy().astype(np.float64)
        worst[key + "_range"] = max(0.0, -val.min(), val.max() - 1)
    _report("T=4200 L=4095", T, worst)
    assert all(x <= _tol(T) for x in worst.values()), worst
    assert (span_skip > 1e-3).sum() > 0
    wide = (torch.zeros((1, 4, 4097), dtype=torch.float32).cuda(), torch.ones((1, 4096), dtype=torch.int32).cuda(),
            torch.tensor([4096], dtype=torch.int32).cuda(), torch.tensor([4], dtype=torch.int32).cuda())
    frames = torch.zeros((1, 4096), dtype=torch.int32).cuda()
    for more in ((), (torch.full((1, 4097), -1, dtype=torch.int32).cuda(),)):
        with pytest.raises(NotImplementedError, match="4095"):
            ops.alignment_posteriors_lattice(*wide, frames, frames, *more)


# ------------------------------------------------------------------------------------------------ A7. the Python surface on the tiny model
@pytest.fixture(scope="module")
def tiny():
    import test_gpu_ragged as tr
    from test_gpu_parity_full import _build
    model, _ = _build("tiny", torch.float32)
    return dict(model=model, tr=tr)


def _sheet_600(model, tr):
    """The 1650-frame, 600-label sheet of tests/test_gpu_wide_lattice.py, rebuilt: lines of 10, every third optional, one onset anchor per
    line at the onset the sheet-only alignment gave the line's first character (or the next sung line's), tolerance 1 s."""
    audio = np.concatenate([tr._clip(4), tr._clip(3)])
    L, n_lines = 600, 60
    ids_all = [int(v) for v in np.random.RandomState(6).randint(2, 403, size=L)]
    labels = torch.tensor([ids_all], dtype=torch.long)
    optional = [i % 3 == 2 for i in range(n_lines)]
    spans = [(10 * i, 10 * i + 10) for i in range(n_lines) if optional[i]]
    sheet_only = model.align([audio], labels, optional_spans=[spans], return_frames=True)
    assert sheet_only[3].tolist() == [0]
    on = sheet_only[0][0].tolist()
    starts, nxt = [0.0] * n_lines, float(1650 - 1) * HOP
    for i in range(n_lines - 1, -1, -1):
        if on[10 * i] >= 0:
            nxt = float(on[10 * i]) * HOP
        starts[i] = nxt
    anchors = [(10 * i, starts[i], 1.0) for i in range(n_lines)]
    return audio, ids_all, labels, optional, spans, starts, anchors


def _score_differences(got, want):
    keys = ("occupancy", "onset_prob", "offset_prob", "sung_prob", "span_skip_prob")
    assert set(got) == set(want) == set(keys) | {"path_log_posterior", "window_log_prob"}
    out = {k: float(np.abs(np.asarray(got[k], np.float64) - np.asarray(want[k], np.float64)).max()) for k in keys if len(want[k])}
    assert all(len(got[k]) == len(want[k]) for k in keys)
    out["path_log_posterior"] = abs(got["path_log_posterior"] - want["path_log_posterior"])
    return out, abs(got["window_log_prob"] - want["window_log_prob"])


def test_a_whole_sheet_of_600_labels_with_its_confidences(tiny):
    from lyricalignment_amd import _lib, ops
    from lyricalignment_amd.harness import PinyinClassLUT, align_record_lrc, align_song
    from lyricalignment_amd.utils import alignment as ua
    from test_gpu_parity_full import VOCAB
    model, tr = tiny["model"], tiny["tr"]
    with torch.no_grad():
        audio, ids_all, labels, optional, spans, starts, anchors = _sheet_600(model, tr)
        L, n_lines = 600, 60
        kw = dict(optional_spans=[spans], onset_anchors=[anchors], skip_penalty=0.5)
        logits, _ = model.frame_manual_forward([audio])
        T = logits.shape[1]
        assert T == 1650
        seconds, scores = model.align([audio], labels, return_sheet_confidence=True, **kw)
        assert seconds == model.align([audio], labels, **kw)
        frames = model.align([audio], labels, return_sheet_confidence=True, return_frames=True, **kw)
        assert len(frames) == 11 and all(torch.is_tensor(t) and t.is_cuda for t in frames) and frames[3].tolist() == [0]
        assert scores[0]["window_log_prob"] == float(frames[7][0] - frames[10][0])
        # the yardstick on the emissions the two-step route computes
        lab_dev, n_lab, lists = ua._labels_to_device(labels, 1, logits.device)
        em = ops.emissions_from_logits(logits.float().contiguous(), lab_dev, n_lab, _lib.LA_VARIANT_CTC)[0].cpu().numpy()
        lo, hi = (w[0].tolist() for w in ua._windows_of(None, [anchors], lists, [T], HOP))
        skip = ua._skip_from_of_spans([spans], lists)[0].tolist()
        dp = wr.viterbi_windows(em, lists[0], lo, hi, skip, 0.5, rows=True)
        assert dp[3] == wr.LA_OK and frames[0][0].tolist() == dp[0] and frames[1][0].tolist() == dp[1]
        gamma, entry, exit_, present, span_skip, log_z = wpr.posteriors(em, lists[0], lo, hi, skip, 0.5)
        log_z_free = wpr.posteriors(em, lists[0], *wr.open_windows(L, T), skip, 0.5)[5]
        occ, onp, offp = spr.scores(gamma, entry, exit_, np.asarray(dp[0]), np.asarray(dp[1]), 2)
        want = dict(occupancy=occ, onset_prob=onp, offset_prob=offp, sung_prob=present, span_skip_prob=[span_skip[n] for _, n in spans],
                    path_log_posterior=dp[2] - log_z, window_log_prob=log_z - log_z_free)
        diff, d_w = _score_differences(scores[0], want)
        print(f"sheet of 600 labels against the yardstick: tol={_tol(T):.2e} " + json.dumps({k: float(f"{x:.2e}") for k, x in diff.items()}) +
              f", window_log_prob {scores[0]['window_log_prob']:.4f} |difference| {d_w:.2e} (tol {2 * _tol(T):.2e})")
        assert all(x <= _tol(T) for x in diff.values()) and d_w <= 2 * _tol(T), (diff, d_w)
        assert scores[0]["window_log_prob"] <= 0.0
        # the function that takes logits
        sec2, sc2 = ua.perform_viterbi_ctc_sheet_scored(logits, labels, **kw)
        assert sec2 == seconds
        diff, d_w = _score_differences(scores[0], sc2[0])
        print("fused against perform_viterbi_ctc_sheet_scored: " + json.dumps({k: float(f"{x:.2e}") for k, x in diff.items()}))
        assert all(x <= _tol(T) for x in diff.values()) and d_w <= 2 * _tol(T), (diff, d_w)
        # the whole song in one call
        lut = PinyinClassLUT([str(i) for i in range(VOCAB)], {str(i): i for i in range(VOCAB)})
        lines = ["".join(chr(0x4E00 + 10 * k + j) for j in range(10)) for k in range(n_lines)]
        ids = {line: ids_all[10 * k: 10 * k + 10] for k, line in enumerate(lines)}
        got, conf = align_song(model, audio, list(zip(starts, lines)), lut, lambda t: ids[t], tolerance_s=1.0, optional=optional, skip_penalty=0.5)
        assert got == align_record_lrc(model, audio, list(zip(starts, lines)), lut, lambda t: ids[t], tolerance_s=1.0, optional=optional,
                                       skip_penalty=0.5)
        assert set(conf) == {"sung", "line_onset_prob", "window_log_prob"} and len(conf["sung"]) == len(conf["line_onset_prob"]) == n_lines
        assert all(abs(conf["sung"][i] - 1.0) <= _tol(T) for i in range(n_lines) if not optional[i])
        assert any(conf["sung"][i] < 1.0 - 1e-3 for i in range(n_lines) if optional[i])
        assert [v is None for v in conf["line_onset_prob"]] == [e is None for e in got]
        assert conf["window_log_prob"] == scores[0]["window_log_prob"] and conf["sung"] == [scores[0]["sung_prob"][10 * i] for i in range(n_lines)]
        plain_lines, conf_lines = align_song(model, audio, lines, lut, lambda t: ids[t], optional=optional, skip_penalty=0.5)
        assert conf_lines["window_log_prob"] == 0.0 and len(plain_lines) == n_lines


def test_on_a_26_label_clip_the_sheet_confidence_is_the_older_keywords_exactly(tiny):
    model, tr = tiny["model"], tiny["tr"]
    audio, labels = tr._clip(4), tr._clip_labels(4)
    spans = [[(0, 3), (10, 20)]]
    with torch.no_grad():
        free = model.align([audio], labels, return_frames=True)
        anchors = [[(12, float(free[0][0, 12]) * HOP + 0.4, 0.2)]]                     # 20 frames off the free onset: the windows bind
        sec, sc = model.align([audio], labels, return_sheet_confidence=True)
        sec_o, sc_o = model.align([audio], labels, return_confidence=True)
        assert sec == sec_o and sc[0]["window_log_prob"] == 0.0 and sc[0]["span_skip_prob"] == [] and sc[0]["sung_prob"] == [1.0] * 26
        assert {k: sc[0][k] for k in sc_o[0]} == sc_o[0]
        sec, sc = model.align([audio], labels, return_sheet_confidence=True, optional_spans=spans, skip_penalty=0.5)
        sec_o, sc_o = model.align([audio], labels, return_span_confidence=True, optional_spans=spans, skip_penalty=0.5)
        assert sec == sec_o and sc[0]["window_log_prob"] == 0.0
        assert {k: x for k, x in sc[0].items() if k != "window_log_prob"} == sc_o[0]
        for sp in (None, spans):
            kw = dict(optional_spans=sp, onset_anchors=anchors, skip_penalty=0.5)
            sec, sc = model.align([audio], labels, return_sheet_confidence=True, **kw)
            sec_o, sc_o = model.align([audio], labels, return_anchored_confidence=True, **kw)
            assert sec == sec_o and sc == sc_o and sc[0]["window_log_prob"] < 0.0
            a = model.align([audio], labels, return_sheet_confidence=True, return_frames=True, **kw)
            b = model.align([audio], labels, return_anchored_confidence=True, return_frames=True, **kw)
            assert len(a) == len(b) == 11 and all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
