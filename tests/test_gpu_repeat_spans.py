"""The alignment DP with repeatable lyric lines on the device (la_viterbi_repeats_batch, ops.viterbi_repeats_batch and the layers over
it): onset, offset, status, path and the float64 score bit for bit against the restatement tests/repeat_spans_reference.py (pinned by
tests/test_host_repeat_spans.py), in every kernel form; a clip alone against the clip in a batch; two calls; nothing repeatable against
la_viterbi_lattice_batch; a prohibitive repeat_penalty; edge spans; repeats with windows and spans; statuses; then the Python surface
on the tiny random-weight model.

Random emissions rarely take a repeat arc, so the emissions are PLANTED from a sung sequence that contains the repetition (the sung cell
-0.25, every other cell -6 minus dyadic noise: ties occur and sums are exact).  That a shape is not vacuous is asserted on the
restatement's path, never on the kernel's."""
import functools

import numpy as np
import pytest
import torch

import repeat_spans_reference as rr
from conftest import e2e_cases
from test_gpu_windows import _labels, _windows_around

pytestmark = pytest.mark.gpu

HOP = 0.02
PEN, RPEN = 0.25, 0.5
KINDS = ("repeat", "both", "declared", "none")


# ------------------------------------------------------------------------------------------------ planted clips
def _plant(rs, T, L, sung, breaths=()):
    """Emissions [T, L+1] for the sung sequence of label indices: every sung label at least one frame, at least one frame of silence in
    front of sung[i] for every i of breaths, the other frames spread at random over the labels' dwell and the silences between and
    around them."""
    assert 0 < len(sung) and len(sung) + len(breaths) <= T
    slots = 2 * len(sung) + 1
    extra = rs.multinomial(T - len(sung) - len(breaths), rs.dirichlet(np.ones(slots)))
    for i in breaths:
        extra[2 * i] += 1
    truth = []
    for i, n in enumerate(sung):
        truth += [0] * int(extra[2 * i]) + [1 + n] * (1 + int(extra[2 * i + 1]))
    truth += [0] * int(extra[-1])
    em = -6.0 - rs.randint(0, 5, size=(T, L + 1)) / 4.0
    em[np.arange(T), truth] = -0.25
    return np.ascontiguousarray(em.astype(np.float32))


def _lines(rs, L):
    bounds = [0]
    while bounds[-1] < L:
        bounds.append(min(L, bounds[-1] + int(rs.randint(1, 7))))
    return list(zip(bounds[:-1], bounds[1:]))


def make_clip(seed, T, L, kind):
    """One planted clip -> dict(lab, em, skip, rf).  A sheet in lines of 1 .. 6 labels with one repeatable line (the chorus) and, for
    "both", one optional line.  kind "repeat": the chorus is sung twice; "both": also the optional line is left out; "declared": arcs
    declared, the sheet sung straight through; "none": nothing declared (null rows)."""
    rs = np.random.RandomState(seed)
    lab = _labels(seed, L)
    lines = _lines(rs, L)
    ci = int(rs.randint(len(lines)))
    oi = None
    if kind in ("both", "declared") and len(lines) >= 2:
        oi = int(rs.choice([i for i in range(len(lines)) if i != ci]))
    skip = rf = None
    if kind != "none":
        rf = [-1] * L
        rf[lines[ci][0]] = lines[ci][1]
        if oi is not None:
            skip = [-1] * (L + 1)
            skip[lines[oi][1]] = lines[oi][0]
    sung, breaths = [], []
    for i, (a, e) in enumerate(lines):
        if kind == "both" and i == oi:
            continue
        sung += list(range(a, e))
        if i == ci and kind in ("repeat", "both"):           # a breath before the chorus comes again: the return through the silence exists
            breaths.append(len(sung))
            sung += list(range(a, e))
    return dict(lab=lab, em=_plant(rs, T, L, sung, breaths), skip=skip, rf=rf, kind=kind)


def reference(c, lo=None, hi=None, pen=PEN, rpen=RPEN):
    return rr.viterbi(c["em"], c["lab"], c["skip"], pen, c["rf"], rpen, lo, hi, rows=True)


# ------------------------------------------------------------------------------------------------ launch
def _launch(clips, pen=PEN, rpen=RPEN, windows=None, null_repeat=False, Tmax=None):
    """Clips of different T / L in ONE la_viterbi_repeats_batch launch -> host arrays (onset, offset, score, status, path).  skip_from is
    null when no clip has a span, repeat_from when no clip has one (or null_repeat); windows: per clip (lo, hi) or None = null windows."""
    from lyricalignment_amd import ops
    B = len(clips)
    Lmax = max(max(len(c["lab"]) for c in clips), 1)
    Tmax = max(c["em"].shape[0] for c in clips) if Tmax is None else Tmax
    em = torch.zeros((B, Tmax, Lmax + 1), dtype=torch.float32)
    labels = torch.zeros((B, Lmax), dtype=torch.int32)
    skip = torch.full((B, Lmax + 1), -1, dtype=torch.int32)
    rf = torch.full((B, Lmax), -1, dtype=torch.int32)
    lo = torch.zeros((B, 2 * Lmax + 1), dtype=torch.int32)
    hi = torch.zeros((B, 2 * Lmax + 1), dtype=torch.int32)
    for b, c in enumerate(clips):
        e, l = c["em"], c["lab"]
        em[b, : e.shape[0], : e.shape[1]] = torch.from_numpy(e)
        labels[b, : len(l)] = torch.tensor(list(l), dtype=torch.int32)
        if c["skip"] is not None:
            skip[b, : len(l) + 1] = torch.tensor(c["skip"], dtype=torch.int32)
        if c["rf"] is not None and len(l):
            rf[b, : len(l)] = torch.tensor(c["rf"], dtype=torch.int32)
        if windows is not None:
            lo[b, : 2 * len(l) + 1] = torch.tensor(windows[b][0], dtype=torch.int32)
            hi[b, : 2 * len(l) + 1] = torch.tensor(windows[b][1], dtype=torch.int32)
    n_labels = torch.tensor([len(c["lab"]) for c in clips], dtype=torch.int32)
    n_frames = torch.tensor([c.get("T", c["em"].shape[0]) for c in clips], dtype=torch.int32)
    any_skip = any(c["skip"] is not None for c in clips)
    any_rf = any(c["rf"] is not None for c in clips) and not null_repeat
    out = ops.viterbi_repeats_batch(em.cuda(), labels.cuda(), n_labels.cuda(), n_frames.cuda(), skip.cuda() if any_skip else None, pen,
                                    lo.cuda() if windows is not None else None, hi.cuda() if windows is not None else None,
                                    rf.cuda() if any_rf else None, rpen)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _assert_equals_reference(got, b, ref, c, what):
    on, off, score, status, path = got
    r_on, r_off, r_score, r_status, r_path = ref
    L, T = len(c["lab"]), c.get("T", c["em"].shape[0])
    print(f"{what}: status {status[b]} / {r_status}, score {float(score[b])!r} / {r_score!r}, repeat arcs {ref.n_repeats}, skip jumps {ref.n_jumps}")
    assert status[b] == r_status, what
    assert on[b, :L].tolist() == r_on and off[b, :L].tolist() == r_off, what
    assert (on[b, L:] == -1).all() and (off[b, L:] == -1).all(), what
    assert np.float64(score[b]).tobytes() == np.float64(r_score).tobytes(), (what, float(score[b]), r_score)
    assert path[b, : len(r_path)].tolist() == r_path and (path[b, len(r_path):] == -1).all(), what
    assert len(r_path) in (0, T), what


def _assert_not_vacuous(clips, refs, what):
    """At least one clip whose reference path takes a repeat arc; where spans are given, one that takes a skip jump AND a repeat arc; one
    with arcs declared and none taken."""
    assert any(r.n_repeats > 0 for r in refs), what
    if any(c["skip"] is not None for c in clips):
        assert any(r.n_repeats > 0 and r.n_jumps > 0 for r in refs), what
    assert any(c["rf"] is not None and r.n_repeats == 0 and r.n_jumps == 0 for c, r in zip(clips, refs)), what


# ------------------------------------------------------------------------------------------------ 1. exact equality, every form
def _mixed(seed, shapes):
    return [make_clip(seed + 13 * i, T, L, KINDS[i % 4]) for i, (T, L) in enumerate(shapes)]


SHAPES = {
    # one wave (S <= 64), in its DPP form and its LDS-exchange form: L 1 .. 31, T 40 .. 120
    "one_wave_dpp": [(40, 1), (57, 7), (64, 12), (41, 2), (120, 31), (90, 26), (77, 19), (48, 3), (100, 31), (113, 30), (66, 5), (80, 4)],
    "one_wave_lds": [(40, 1), (57, 7), (64, 12), (41, 2), (120, 31), (90, 26), (77, 19), (48, 3), (100, 31), (113, 30), (66, 5), (80, 4)],
    "2_waves_L33": [(90, 33), (80, 33), (70, 32), (50, 9)],
    "4_waves_L100": [(160, 100), (150, 97), (131, 100), (90, 40)],
    "8_waves_L200": [(300, 200), (280, 200), (260, 170), (100, 33)],
    "16_waves_L511": [(640, 511), (650, 511), (620, 480), (200, 100)],
    "masks_leave_lds_T7000_L20": [(300, 20), (7000, 20), (6100, 17), (300, 9)],
    "strip_R2_L512": [(640, 512), (640, 512), (630, 505), (200, 100)],
    "strip_R2_L1023": [(1280, 1023), (1290, 1023), (700, 520), (200, 100)],
    "strip_R4_L1024": [(1280, 1024), (1290, 1024), (700, 520), (200, 100)],
    "strip_R8_L2048": [(1000, 800), (2560, 2048), (700, 520), (200, 100)],
    "strip_R8_L4095": [(1000, 800), (5120, 4095), (700, 520), (200, 100)],
}


@functools.lru_cache(maxsize=None)
def reference_cases(name):
    """The clips of one shape with their yardstick results, computed once on the host."""
    clips = _mixed(sum(map(ord, name)), SHAPES[name])
    return clips, [reference(c) for c in clips]


@pytest.mark.parametrize("name", list(SHAPES))
def test_equals_the_float64_reference_exactly(name):
    """Per shape one launch of clips of different lengths: the chorus sung twice; the chorus sung twice and an optional line left out;
    arcs declared and the sheet sung straight through; nothing declared."""
    from lyricalignment_amd import _lib
    clips, refs = reference_cases(name)
    _assert_not_vacuous(clips, refs, name)
    assert all(r[3] == rr.LA_OK for r in refs)
    with _lib.option("viterbi_dpp", 0 if name == "one_wave_lds" else 1):
        got = _launch(clips)
    for b, (c, r) in enumerate(zip(clips, refs)):
        _assert_equals_reference(got, b, r, c, (name, b, c["kind"]))


# ------------------------------------------------------------------------------------------------ 2. alone = in a batch; two calls
@pytest.mark.parametrize("name", ["one_wave_dpp", "4_waves_L100", "strip_R2_L512"])
def test_a_clip_alone_equals_the_clip_in_a_batch_and_two_calls_agree(name):
    clips, refs = reference_cases(name)
    first, second = _launch(clips), _launch(clips)
    for x, y in zip(first, second):
        assert x.tobytes() == y.tobytes()
    for b, c in enumerate(clips[:5]):
        alone = _launch([c])
        _assert_equals_reference(alone, 0, refs[b], c, (name, b, "alone"))
        L, T = len(c["lab"]), c["em"].shape[0]
        assert alone[0][0, :L].tolist() == first[0][b, :L].tolist() and alone[1][0, :L].tolist() == first[1][b, :L].tolist()
        assert alone[2][0].tobytes() == first[2][b].tobytes() and alone[3][0] == first[3][b]
        assert alone[4][0, :T].tolist() == first[4][b, :T].tolist()


# ------------------------------------------------------------------------------------------------ 3. nothing repeatable = the lattice entry
def _same_as_lattice(em, labels, n_lab, n_fr, skip, pen, lo, hi, what):
    from lyricalignment_amd import ops
    want = ops.viterbi_lattice_batch(em, labels, n_lab, n_fr, skip, pen, lo, hi)
    none = torch.full((labels.shape[0], labels.shape[1]), -1, dtype=torch.int32).cuda()
    outs = [ops.viterbi_repeats_batch(em, labels, n_lab, n_fr, skip, pen, lo, hi, rf, 0.5) for rf in (None, none)]
    for got in outs:
        for name, w, g in zip(("onset", "offset", "score", "status"), want, got):
            assert torch.equal(w, g), (what, name)
        assert want[2].cpu().numpy().tobytes() == got[2].cpu().numpy().tobytes(), what
    assert torch.equal(outs[0][4], outs[1][4])
    return want, outs[0][4]


def test_null_and_all_minus_one_repeat_from_equal_the_lattice_entry_on_the_golden_cases():
    n = 0
    for m, b, em, label, seconds in e2e_cases():
        em_d = torch.from_numpy(np.ascontiguousarray(em, dtype=np.float32))[None].cuda()
        L, T = len(label), em.shape[0]
        labels = torch.tensor([[int(v) for v in label]], dtype=torch.int32).cuda()
        want, path = _same_as_lattice(em_d, labels, torch.tensor([L], dtype=torch.int32).cuda(), torch.tensor([T], dtype=torch.int32).cuda(),
                                      None, 0.0, None, None, (m["name"], b))
        if int(want[3][0]) == 0:                     # the path's first visits are the onsets (the plain lattice visits every label once)
            seg = rr.segments(path[0].tolist())
            assert [s[1] for s in seg] == want[0][0, :L].tolist() and [s[2] for s in seg] == want[1][0, :L].tolist()
        n += 1
    assert n > 0


@pytest.mark.parametrize("T,L", [(90, 31), (300, 100), (700, 600), (2300, 2100)])
def test_null_and_all_minus_one_repeat_from_equal_the_lattice_entry_with_spans_and_windows(T, L):
    from test_gpu_wide_lattice import _sheet
    from test_gpu_windows import _emissions
    lab = _labels(5, L)
    ems = [_emissions(1, T, lab, 0.0), _emissions(2, T, lab, 1.5)]
    em = torch.from_numpy(np.ascontiguousarray(np.stack(ems))).cuda()
    labels = torch.tensor([lab] * 2, dtype=torch.int32).cuda()
    n_lab, n_fr = torch.full((2,), L, dtype=torch.int32).cuda(), torch.full((2,), T, dtype=torch.int32).cuda()
    skip = torch.tensor([_sheet(9, L)] * 2, dtype=torch.int32).cuda()
    free, path = _same_as_lattice(em, labels, n_lab, n_fr, skip, 0.25, None, None, "spans")
    assert (free[3] == 0).all() and int((free[0] < 0).sum()) > 0
    _same_as_lattice(em, labels, n_lab, n_fr, None, 0.0, None, None, "nothing")
    rs = np.random.RandomState(T + L)
    paths = path.cpu().numpy()
    wins = [_windows_around(rs, paths[1 - b].tolist(), 2 * L + 1, T) for b in range(2)]          # each clip: around the OTHER clip's path
    lo = torch.tensor([w[0] for w in wins], dtype=torch.int32).cuda()
    hi = torch.tensor([w[1] for w in wins], dtype=torch.int32).cuda()
    bound, _ = _same_as_lattice(em, labels, n_lab, n_fr, skip, 0.25, lo, hi, "spans + windows")
    _same_as_lattice(em, labels, n_lab, n_fr, None, 0.0, lo, hi, "windows")
    assert not torch.equal(bound[0], free[0])                                                    # the windows bind


# ------------------------------------------------------------------------------------------------ 4. a prohibitive penalty
@pytest.mark.parametrize("name", ["one_wave_dpp", "8_waves_L200", "strip_R4_L1024"])
def test_a_prohibitive_repeat_penalty_gives_the_repeat_free_result(name):
    """repeat_penalty = 1e9 lies below every finite cell (the initial value is -1e7), so no repeat arc ever wins a strict comparison: the
    outputs are those of the same launch without repeat_from, and la_viterbi_lattice_batch's."""
    clips, _ = reference_cases(name)
    barred = _launch(clips, rpen=1e9)
    free = _launch(clips, null_repeat=True)
    for x, y in zip(barred, free):
        assert x.tobytes() == y.tobytes()
    refs = [rr.viterbi(c["em"], c["lab"], c["skip"], PEN, None, 0.0, rows=True) for c in clips[:4]]
    for b, r in enumerate(refs):
        _assert_equals_reference(barred, b, r, clips[b], (name, b, "barred"))
    assert any(r[3] != rr.LA_OK or tuple(r) != tuple(w) for r, w in zip(refs, reference_cases(name)[1]))      # the repeats mattered


# ------------------------------------------------------------------------------------------------ 5. edge spans
def _edge_clip(lab, rf, skip, sung, T, seed):
    rs = np.random.RandomState(seed)
    breaths = [i for i in range(1, len(sung)) if sung[i] <= sung[i - 1]]                     # a breath before every return
    return dict(lab=lab, em=_plant(rs, T, len(lab), sung, breaths), skip=skip, rf=rf, kind="edge")


EDGES = {
    "a=0": ([1, 2, 3, 4, 5], [3, -1, -1, -1, -1], None, [0, 1, 2, 0, 1, 2, 3, 4]),
    "e=L": ([1, 2, 3, 4, 5], [-1, -1, 5, -1, -1], None, [0, 1, 2, 3, 4, 2, 3, 4]),
    "whole sheet": ([1, 2, 3], [3, -1, -1], None, [0, 1, 2, 0, 1, 2, 0, 1, 2]),
    "one-label span": ([1, 2, 3], [-1, 2, -1], None, [0, 1, 1, 1, 2]),
    "one label": ([4], [1], None, [0, 0, 0]),
    "equal labels at both ends": ([1, 2, 3, 2, 5], [-1, 4, -1, -1, -1], None, [0, 1, 2, 3, 1, 2, 3, 4]),
    "nested": ([1, 2, 3, 4, 5, 6], [-1, 5, 4, -1, -1, -1], None, [0, 1, 2, 3, 2, 3, 4, 1, 2, 3, 4, 5]),
    "overlapping": ([1, 2, 3, 4, 5, 6], [-1, 4, -1, 6, -1, -1], None, [0, 1, 2, 3, 1, 2, 3, 4, 5, 3, 4, 5]),
    "visit beats skip": ([1, 2, 3, 4], [3, -1, -1, -1], [-1, -1, 1, -1, -1], [0, 2, 0, 1, 2, 3]),
    "chorus after the verse": ([1, 2, 3, 4, 5, 6], [-1, -1, 6, -1, -1, -1], [-1, -1, -1, -1, -1, -1, 4], [0, 1, 2, 3, 4, 5, 2, 3]),
}


@pytest.mark.parametrize("dpp", [1, 0])
def test_edge_spans(dpp):
    from lyricalignment_amd import _lib
    clips = [_edge_clip(lab, rf, skip, sung, 50 + 3 * i, i) for i, (lab, rf, skip, sung) in enumerate(EDGES.values())]
    refs = [reference(c, pen=0.0, rpen=0.25) for c in clips]
    for name, c, r, (_, _, _, sung) in zip(EDGES, clips, refs, EDGES.values()):
        assert r[3] == rr.LA_OK and [n for n, _, _ in rr.segments(r[4])] == sung, name          # the planted sequence, visit by visit
        assert r.n_repeats == sum(1 for x, y in zip(sung, sung[1:]) if y <= x), name
    assert refs[8].n_jumps == 1 and refs[8][0][1] >= 0                                          # skipped on one pass, visited on another
    with _lib.option("viterbi_dpp", dpp):
        got = _launch(clips, pen=0.0, rpen=0.25)
    for b, (name, c, r) in enumerate(zip(EDGES, clips, refs)):
        _assert_equals_reference(got, b, r, c, (name, dpp))


def test_visit_beats_skip_in_the_strip_kernel():
    """520 labels: label 1 optional, labels 0 .. 2 repeatable, the audio sings 0 2 0 1 2 3 ...: label 1 has its visit's onset."""
    L = 520
    lab = _labels(3, L)
    lab[:4] = [1, 2, 3, 4]
    rf, skip = [-1] * L, [-1] * (L + 1)
    rf[0], skip[2] = 3, 1
    c = _edge_clip(lab, rf, skip, [0, 2, 0, 1, 2] + list(range(3, L)), 700, 1)
    r = reference(c, pen=0.0, rpen=0.25)
    assert r[3] == rr.LA_OK and r.n_jumps == 1 and r.n_repeats == 1 and r[0][1] > r[0][2]
    _assert_equals_reference(_launch([c], pen=0.0, rpen=0.25), 0, r, c, "strip")


# ------------------------------------------------------------------------------------------------ 6. repeats with windows and spans
@pytest.mark.parametrize("name", ["one_wave_dpp", "one_wave_lds", "4_waves_L100", "strip_R2_L512"])
def test_repeats_with_windows_and_spans(name):
    """Every clip's windows lie around its own unwindowed path and keep its score -- except in the clips that sing the chorus twice, where
    the one window that is not open lets a label that is visited once, for two frames or more, be entered only one frame later: the
    window binds, and the restatement still takes the repeat arc."""
    from lyricalignment_amd import _lib
    clips, free = reference_cases(name)
    rs = np.random.RandomState(len(name))
    wins, bound = [], []
    for c, r in zip(clips, free):
        T, S = c["em"].shape[0], 2 * len(c["lab"]) + 1
        lo, hi = _windows_around(rs, r[4], S, T)
        seg = rr.segments(r[4])
        once = [v for v in seg if sum(1 for w in seg if w[0] == v[0]) == 1 and v[2] - v[1] >= 2]
        bound.append(r.n_repeats > 0 and bool(once))
        if bound[-1]:                                  # (every other window open: the states before it can wait the extra frame)
            lo, hi = [0] * S, [T] * S
            lo[2 * once[0][0] + 1] = once[0][1] + 1
        wins.append((lo, hi))
    refs = [reference(c, *w) for c, w in zip(clips, wins)]
    assert any(bound)
    for r, f, bnd in zip(refs, free, bound):
        assert r[3] == rr.LA_OK
        assert (r[0], r[1]) != (f[0], f[1]) if bnd else r[2] == f[2]          # (not bound: the best score survives; ties may pick another path)
    assert any(r.n_repeats > 0 and bnd for r, bnd in zip(refs, bound))
    assert any(r.n_repeats > 0 and r.n_jumps > 0 for r in refs)
    with _lib.option("viterbi_dpp", 0 if name == "one_wave_lds" else 1):
        got = _launch(clips, windows=wins)
    for b, (c, r) in enumerate(zip(clips, refs)):
        _assert_equals_reference(got, b, r, c, (name, b, "windows"))


# ------------------------------------------------------------------------------------------------ 7. statuses
@pytest.mark.parametrize("Lmax", [26, 600])
def test_statuses_and_the_path_of_a_clip_without_a_backtrace(Lmax):
    ok = make_clip(1, 60 if Lmax == 26 else 800, Lmax, "repeat")
    short = make_clip(2, 60, 20, "repeat")
    short["T"] = 7                                                       # 20 labels in 7 frames: too short
    empty = dict(lab=[], em=np.zeros((5, 1), dtype=np.float32), skip=None, rf=None, kind="empty")
    no_frames = dict(make_clip(3, 30, 8, "declared"), T=0)
    closed = make_clip(4, 50, 9, "repeat")
    clips = [ok, short, empty, no_frames, closed]
    wins = [rr._open(None, None, 2 * len(c["lab"]) + 1, c["em"].shape[0]) for c in clips]
    wins[4] = ([1] * 19, wins[4][1])                                     # row 0 closed: no path inside the windows
    got = _launch(clips, windows=wins)
    on, off, score, status, path = got
    r_ok = reference(ok)
    _assert_equals_reference(got, 0, r_ok, ok, "ok")
    assert r_ok.n_repeats > 0
    r_short = rr.viterbi(short["em"][:7], short["lab"], short["skip"], PEN, short["rf"], RPEN)
    assert r_short[3] == rr.LA_EINFEASIBLE
    _assert_equals_reference(got, 1, r_short, short, "too short")
    assert (path[1, 7:] == -1).all() and (path[1, :7] >= 0).all()
    assert status[2] == rr.LA_EEMPTY and status[3] == rr.LA_EINVAL and score[2] == 0.0 and score[3] == 0.0
    r_closed = reference(closed, *wins[4])
    assert r_closed[3] == rr.LA_EINFEASIBLE and r_closed[2] == rr.NINF and r_closed[4] == []
    _assert_equals_reference(got, 4, r_closed, closed, "no path inside the windows")
    for b in (2, 3, 4):
        assert (path[b] == -1).all() and (on[b] == -1).all() and (off[b] == -1).all()


def test_wrapper_refusals():
    from lyricalignment_amd import ops
    em = torch.zeros((2, 30, 9), dtype=torch.float32).cuda()
    lab = torch.ones((2, 8), dtype=torch.int32).cuda()
    n, t = torch.full((2,), 8, dtype=torch.int32).cuda(), torch.full((2,), 30, dtype=torch.int32).cuda()
    rf = torch.full((2, 8), -1, dtype=torch.int32).cuda()
    for bad in (rf[:1], rf[:, :7], rf.long(), rf.cpu()):
        with pytest.raises(ValueError):
            ops.viterbi_repeats_batch(em, lab, n, t, repeat_from=bad)
    for pen in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            ops.viterbi_repeats_batch(em, lab, n, t, repeat_from=rf, repeat_penalty=pen)
    with pytest.raises(ValueError):
        ops.viterbi_repeats_batch(em, lab, n, t, win_lo=torch.zeros((2, 17), dtype=torch.int32).cuda())
    with pytest.raises(NotImplementedError):
        ops.viterbi_repeats_batch(torch.zeros((1, 4, 4097), dtype=torch.float32).cuda(), torch.ones((1, 4096), dtype=torch.int32).cuda(),
                                  n[:1], t[:1])
    assert len(ops.viterbi_repeats_batch(em, lab, n, t)) == 5


# ------------------------------------------------------------------------------------------------ 8. the Python surface
def _planted_logits(classes_sung, T, width, seg):
    """CTC-variant logits [1, T, width] (column c = class c, the last column = the silence logit) for a sung sequence of classes."""
    lg = torch.full((1, T, width), -4.0)
    lg[:, :, -1] = 6.0
    t = seg
    for c in classes_sung:
        lg[0, t: t + seg, c] = 6.0
        lg[0, t: t + seg, -1] = -6.0
        t += 2 * seg
    assert t <= T
    return lg


def test_perform_viterbi_ctc_finds_both_occurrences_on_planted_logits():
    from lyricalignment_amd.utils import alignment as ua
    labels = torch.tensor([[3, 5, 7, 2, 9, 4]])                      # lines: (3 5) (7 2) (9 4); the audio sings A B B C
    sung = [3, 5, 7, 2, 7, 2, 9, 4]
    lg = _planted_logits(sung, 5 * (2 * len(sung) + 1), 12, 5).cuda()
    seconds, segments = ua.perform_viterbi_ctc(lg, labels, repeat_spans=[[(2, 4)]], repeat_penalty=1.0, return_segments=True)
    assert [n for n, _, _ in segments[0]] == [0, 1, 2, 3, 2, 3, 4, 5]
    assert [(round(a / HOP), round(b / HOP)) for _, a, b in segments[0]] == [(5 + 10 * i, 10 + 10 * i) for i in range(8)]
    assert seconds[0] == [[a, b] for n, a, b in segments[0][:4] + segments[0][6:]]             # the first visit per character
    assert seconds == ua.perform_viterbi_ctc(lg, labels, repeat_spans=[[(2, 4)]], repeat_penalty=1.0)
    # without the keywords: the call as it was; with return_segments alone: its result and one visit per character
    plain = ua.perform_viterbi_ctc(lg, labels)
    assert ua.perform_viterbi_ctc(lg, labels, repeat_spans=None) == plain and ua.perform_viterbi_ctc(lg, labels, repeat_spans=[[]]) == plain
    same, seg = ua.perform_viterbi_ctc(lg, labels, return_segments=True)
    assert same == plain and [[a, b] for _, a, b in seg[0]] == plain[0] and [n for n, _, _ in seg[0]] == list(range(6))
    assert plain != seconds
    # a chorus that returns after the verse: a repeat span over chorus .. verse plus that verse optional
    sung = [3, 5, 7, 2, 9, 4, 7, 2]
    lg = _planted_logits(sung, 5 * (2 * len(sung) + 1), 12, 5).cuda()
    seconds, segments = ua.perform_viterbi_ctc(lg, labels, repeat_spans=[[(2, 6)]], optional_spans=[[(4, 6)]], return_segments=True)
    assert [n for n, _, _ in segments[0]] == [0, 1, 2, 3, 4, 5, 2, 3] and None not in seconds[0]
    # refusals: bad spans, any confidence, the training loss
    for bad in ([[(2, 2)]], [[(0, 7)]], [[(-1, 2)]], [[(1, 3), (1, 4)]], [[], []]):
        with pytest.raises(ValueError):
            ua.perform_viterbi_ctc(lg, labels, repeat_spans=bad)
    for scored in (ua.perform_viterbi_ctc_scored, ua.perform_viterbi_scored, ua.perform_viterbi_ctc_anchored_scored, ua.perform_viterbi_ctc_sheet_scored):
        with pytest.raises(ValueError):
            scored(lg, labels, repeat_spans=[[(2, 4)]])
    with pytest.raises(ValueError):
        ua.anchored_alignment_loss(lg, labels, repeat_spans=[[(2, 4)]])
    with pytest.raises(ValueError):
        ua.run_lattice(*[None] * 4, confidence="plain", repeat_from=torch.zeros((1, 6), dtype=torch.int32))


@pytest.fixture(scope="module")
def tiny():
    import test_gpu_ragged as tr
    from test_gpu_parity_full import _build
    model, _ = _build("tiny", torch.float32)
    idx = [0, 1, 3, 5]                                           # clips of tests/test_gpu_ragged.py: 11, 5, 8, 3 labels
    return dict(model=model, audios=[tr._clip(i) for i in idx], labels=tr._padded_labels(idx), tr=tr, idx=idx)


REPEATS = [[(3, 7), (0, 2)], [(0, 5)], [(2, 3)], []]
OPTIONAL = [[(7, 9)], [], [(5, 8)], []]


@pytest.mark.parametrize("use_ctc", [True, False])
def test_align_with_repeats_equals_the_two_step_route(tiny, use_ctc):
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels = tiny["model"], tiny["audios"], tiny["labels"]
    two = ua.perform_viterbi_ctc if use_ctc else ua.perform_viterbi
    with torch.no_grad():
        logits, _ = model.frame_manual_forward(audios)
        n_visits = []
        for kw in (dict(repeat_spans=REPEATS), dict(repeat_spans=REPEATS, repeat_penalty=2.0),
                   dict(repeat_spans=REPEATS, optional_spans=OPTIONAL, skip_penalty=0.5),
                   dict(repeat_spans=REPEATS, onset_anchors=[[(4, 1.0, 0.5)], [], [], []])):
            fused = model.align(audios, labels, use_ctc=use_ctc, return_segments=True, **kw)
            assert fused == two(logits, labels, return_segments=True, **kw)
            assert fused[0] == model.align(audios, labels, use_ctc=use_ctc, **kw)
            frames = model.align(audios, labels, use_ctc=use_ctc, return_frames=True, **kw)
            assert len(frames) == 5 and frames[3].tolist() == [0] * 4 and frames[4].dtype == torch.int32
            for b, (res, seg) in enumerate(zip(*fused)):
                firsts = {}
                for n, a, e in seg:
                    firsts.setdefault(n, [a, e])
                assert res == [firsts.get(n) for n in range(len(res))]
                assert seg == [(n, f * HOP, e * HOP) for n, f, e in rr.segments(frames[4][b].tolist())]
            n_visits.append([len(seg) for seg in fused[1]])
        print(f"use_ctc={use_ctc}: visits per clip {n_visits}")
        plain = model.align(audios, labels, use_ctc=use_ctc)
        assert model.align(audios, labels, use_ctc=use_ctc, repeat_spans=None) == plain
        assert model.align(audios, labels, use_ctc=use_ctc, repeat_spans=[[], [], [], []]) == plain
        assert model.align(audios, labels, use_ctc=use_ctc, return_segments=True)[0] == plain
        for kw in (dict(return_confidence=True), dict(return_span_confidence=True), dict(return_anchored_confidence=True),
                   dict(return_sheet_confidence=True)):
            with pytest.raises(ValueError):
                model.align(audios, labels, repeat_spans=REPEATS, **kw)


def test_per_clip_and_long_form_with_repeats(tiny):
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels, tr = tiny["model"], tiny["audios"], tiny["labels"], tiny["tr"]
    with torch.no_grad():
        batch = model.align(audios, labels, per_clip=True, repeat_spans=REPEATS, return_segments=True)
        for r, i in enumerate(tiny["idx"]):
            alone = model.align([audios[r]], tr._clip_labels(i), per_clip=True, repeat_spans=[REPEATS[r]], return_segments=True)
            assert batch[0][r] == alone[0][0] and batch[1][r] == alone[1][0], i
        audio = np.concatenate([tr._clip(4), tr._clip(3)])                                     # 33 s: two encoder chunks
        lab = torch.from_numpy(np.random.RandomState(5).randint(2, 403, size=(1, 14)))
        kw = dict(repeat_spans=[[(3, 7)]], optional_spans=[[(10, 14)]], return_segments=True)
        logits, _ = model.frame_manual_forward([audio])
        assert logits.shape[1] > 1500
        assert model.align([audio], lab, **kw) == ua.perform_viterbi_ctc(logits, lab, **kw)


def test_align_record_lines_lists_every_occurrence(tiny):
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
    optional, repeatable = [False, False, True, False], [False, True, False, True]
    got = align_record_lines(model, tr._clip(0), lines, optional, lut, lambda t: ids[t], repeatable=repeatable, repeat_penalty=0.0)
    with torch.no_grad():
        _, seg = model.align([tr._clip(0)], tr._clip_labels(0), optional_spans=[[(7, 9)]], repeat_spans=[[(3, 7), (9, 11)]],
                             return_segments=True)
    assert len(got) == 4 and all(isinstance(e, list) for e in got)
    flat = sorted((c[0], c[1], c[2]) for occ in got for o in occ for c in o)
    starts = [0, 3, 7, 9]
    line_of = [i for i, line in enumerate(lines) for _ in line]
    assert flat == sorted((a, e, lines[line_of[n]][n - starts[line_of[n]]]) for n, a, e in seg[0])
    for i, occ in enumerate(got):
        for o in occ:
            assert [c[2] for c in o] == list(lines[i])[: len(o)] or "".join(c[2] for c in o) in lines[i]
            assert all(x[1] <= y[0] for x, y in zip(o, o[1:]))
    print(f"occurrences per line {[len(o) for o in got]}")
    assert align_record_lines(model, tr._clip(0), lines, optional, lut, lambda t: ids[t]) is not None      # repeatable None: as before
    with pytest.raises(ValueError):
        align_record_lines(model, tr._clip(0), lines, optional, lut, lambda t: ids[t], repeatable=repeatable, with_confidence=True)
    with pytest.raises(ValueError):
        align_record_lines(model, tr._clip(0), lines, optional, lut, lambda t: ids[t], repeatable=[True])
