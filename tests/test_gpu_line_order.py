"""The alignment DP with free line order on the device (la_viterbi_lines_batch, ops.viterbi_lines_batch and the layers over it): onset,
offset, path, status and the float64 score bit for bit against the all-pairs restatement tests/line_order_reference.py (pinned by
tests/test_host_line_order.py) in every kernel form; a clip alone against the clip in a batch; two calls; penalty +inf against
la_viterbi_batch; one line against la_viterbi_repeats_batch; the equal-class rule; statuses; then the Python surface on the tiny
random-weight model and the bench tool.

Emissions are PLANTED from a sung order of lines plus continuous noise (ties have measure zero), and that a shape is not vacuous -- at
least two jumps, an unvisited line, a free start or end -- is asserted on the restatement's path before the device is compared."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import line_order_reference as lo
from conftest import ROOT

pytestmark = pytest.mark.gpu

HOP = 0.02
PEN = 1.0

# labels x frames -> (line lengths, the lines sung in order, frames per label, frames of silence after a line); the kernel form in the id
SHAPES = {
    "one_wave_5x24": (24, [2, 3], [1, 1, 1], 2, 1),
    # labels 0 .. 31 lie in wave 0: line 3 ends in state 63 (wave 0) / 64 (wave 1) and line 4 starts in wave 1.  Sung: a free start at
    # line 1, a backward jump to line 0, a forward jump over line 1, one over line 3, and line 4 again
    "two_waves_40x200": (200, [8] * 5, [1, 0, 2, 4, 4], 4, 2),
    "nw16_300x700": (700, [30] * 10, [2, 0, 1, 1, 3, 5], 3, 2),
    "r2_600x1400": (1400, [30] * 20, [3, 4, 5, 1, 2, 2, 7, 8, 9, 10, 12], 4, 2),
    "r4_1100x2400": (2400, [22] * 50, list(range(5, 25)) + list(range(2, 20)) + [19] + list(range(30, 40)), 2, 1),
    "r8_2100x4400": (4400, [21] * 100, list(range(10, 50)) + list(range(5, 45)) + [44] + list(range(80, 98)), 2, 1),
}


@functools.lru_cache(maxsize=None)
def clip_and_reference(name, pen=PEN):
    T, lengths, sung, seg, gap = SHAPES[name]
    c = lo.planted(len(name), T, lengths, sung, seg, gap)
    return c, lo.viterbi(c["em"], c["lab"], c["ls"], pen)


def _launch(clips, pen=PEN, Tmax=None):
    """Clips of different T / L in ONE la_viterbi_lines_batch launch -> host arrays (onset, offset, score, status, path)."""
    from lyricalignment_amd import ops
    B = len(clips)
    Lmax = max(max(len(c["lab"]) for c in clips), 1)
    Tmax = max(c["em"].shape[0] for c in clips) if Tmax is None else Tmax
    em = torch.zeros((B, Tmax, Lmax + 1), dtype=torch.float32)
    labels = torch.zeros((B, Lmax), dtype=torch.int32)
    ls = torch.zeros((B, Lmax), dtype=torch.int32)
    for b, c in enumerate(clips):
        e, l = c["em"], c["lab"]
        em[b, : e.shape[0], : e.shape[1]] = torch.from_numpy(e)
        labels[b, : len(l)] = torch.tensor(list(l), dtype=torch.int32)
        ls[b, : len(l)] = torch.tensor(c["ls"], dtype=torch.int32)
    n_labels = torch.tensor([len(c["lab"]) for c in clips], dtype=torch.int32)
    n_frames = torch.tensor([c["T"] for c in clips], dtype=torch.int32)
    out = ops.viterbi_lines_batch(em.cuda(), labels.cuda(), n_labels.cuda(), n_frames.cuda(), ls.cuda(), pen)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _assert_equals_reference(got, b, ref, c, what):
    on, off, score, status, path = got
    r_on, r_off, r_score, r_status, r_path = ref
    L, T = len(c["lab"]), c["T"]
    print(f"{what}: status {status[b]} / {r_status}, score {float(score[b])!r} / {r_score!r}, jumps {ref.n_jumps}, free start {ref.free_start}, "
          f"free end {ref.free_end}")
    assert status[b] == r_status, what
    assert np.float64(score[b]).tobytes() == np.float64(r_score).tobytes(), (what, float(score[b]), r_score)
    assert path[b, : len(r_path)].tolist() == r_path and (path[b, len(r_path):] == -1).all(), what
    assert on[b, :L].tolist() == r_on and off[b, :L].tolist() == r_off, what
    assert (on[b, L:] == -1).all() and (off[b, L:] == -1).all(), what
    assert len(r_path) in (0, T), what


def _assert_not_vacuous(c, ref, what):
    """On the restatement alone: at least two jumps, a line never visited, a free start or a free end."""
    L = len(c["lab"])
    order = lo.line_order(ref[4], c["ls"], L)
    n_lines = len(lo.line_starts_of(c["ls"], L))
    assert ref[3] == lo.LA_OK and ref.n_jumps >= 2, (what, ref.n_jumps)
    assert set(order) != set(range(n_lines)), what
    assert ref.free_start or ref.free_end, what
    return order


# ------------------------------------------------------------------------------------------------ 1. the restatement, every kernel form
@pytest.mark.parametrize("name", list(SHAPES))
def test_device_equals_the_all_pairs_restatement(name):
    c, ref = clip_and_reference(name)
    order = _assert_not_vacuous(c, ref, name)
    assert order == c["sung"], (name, order)           # the planted performance is what the restatement finds
    _assert_equals_reference(_launch([c]), 0, ref, c, name)


@pytest.mark.parametrize("pen", [0.0, 0.3])
def test_random_emissions_with_few_classes_jump_all_the_time(pen):
    """Unplanted noise over a two-class alphabet: hundreds of jumps, equal classes between line ends and line starts everywhere, one
    wave, two waves and sixteen."""
    clips = []
    for seed, (L, T, n_lines) in enumerate(((9, 60, 4), (40, 200, 9), (300, 240, 40))):
        rs = np.random.RandomState(100 + seed)
        cuts = sorted(rs.choice(np.arange(1, L), size=n_lines - 1, replace=False).tolist())
        lengths = np.diff([0] + cuts + [L]).tolist()
        c = lo.planted(seed, T, lengths, [], vocab=2)
        c["em"] = np.ascontiguousarray(np.log(rs.dirichlet(np.ones(L + 1), size=T)).astype(np.float32))
        clips.append(c)
    refs = [lo.viterbi(c["em"], c["lab"], c["ls"], pen) for c in clips]
    assert all(r.n_jumps >= 5 for r in refs), [r.n_jumps for r in refs]
    got = _launch(clips, pen)
    for b, (c, r) in enumerate(zip(clips, refs)):
        _assert_equals_reference(got, b, r, c, f"random clip {b} penalty {pen}")


# ------------------------------------------------------------------------------------------------ 2. ragged batch, two calls, untouched cells
def test_a_clip_in_a_ragged_batch_equals_the_clip_alone_and_two_calls_agree():
    names = ["one_wave_5x24", "nw16_300x700", "two_waves_40x200"]
    clips = [clip_and_reference(n)[0] for n in names]
    refs = [clip_and_reference(n)[1] for n in names]
    batch = _launch(clips)
    again = _launch(clips)
    for x, y in zip(batch, again):
        assert x.tobytes() == y.tobytes()
    for b, (c, r, n) in enumerate(zip(clips, refs, names)):
        _assert_equals_reference(batch, b, r, c, f"{n} in the batch")         # (also: every cell beyond L_b / T_b holds -1)
        alone = _launch([c], Tmax=batch[4].shape[1])
        L, T = len(c["lab"]), c["T"]
        assert alone[0][0, :L].tolist() == batch[0][b, :L].tolist() and alone[1][0, :L].tolist() == batch[1][b, :L].tolist()
        assert alone[2][0].tobytes() == batch[2][b].tobytes() and alone[4][0, :T].tolist() == batch[4][b, :T].tolist()


# ------------------------------------------------------------------------------------------------ 3. the two identities
def test_an_infinite_penalty_is_the_plain_lattice():
    from lyricalignment_amd import ops
    for name in ("two_waves_40x200", "r2_600x1400"):
        T, lengths, _, seg, gap = SHAPES[name]
        c = lo.planted(7, T, lengths, list(range(len(lengths))), 1, 0)            # sung straight through: the plain lattice has a path
        got = _launch([c], float("inf"))
        L = len(c["lab"])
        em = torch.from_numpy(c["em"])[None].cuda()
        want = ops.viterbi_batch(em, torch.tensor([c["lab"]], dtype=torch.int32).cuda(), torch.tensor([L], dtype=torch.int32).cuda(),
                                 torch.tensor([T], dtype=torch.int32).cuda())
        torch.cuda.synchronize()
        on, off, score, status = (t.cpu().numpy() for t in want)
        assert status[0] == lo.LA_OK and got[3][0] == lo.LA_OK
        assert got[0].tobytes() == on.tobytes() and got[1].tobytes() == off.tobytes() and got[2].tobytes() == score.tobytes(), name
        assert (np.diff(got[4][0]) >= 0).all() and (np.diff(got[4][0]) <= 2).all()


@pytest.mark.parametrize("L,T", [(26, 300), (600, 1400)])
def test_a_single_line_is_the_repeat_lattice_with_the_whole_sheet_repeatable(L, T):
    from lyricalignment_amd import ops
    seg = 3 if L == 26 else 1
    # the sheet sung twice (one frame per label at 600 x 1400: no equal neighbours, which would need a frame of silence between them)
    c = lo.planted(L, T, [L], [0, 0], seg, 2, labels=[1 + n % 37 for n in range(L)])
    ref = lo.viterbi(c["em"], c["lab"], c["ls"], 0.5)
    assert ref.n_jumps >= 1
    got = _launch([c], 0.5)
    _assert_equals_reference(got, 0, ref, c, f"one line {L} x {T}")
    rf = torch.full((1, L), -1, dtype=torch.int32)
    rf[0, 0] = L
    want = ops.viterbi_repeats_batch(torch.from_numpy(c["em"])[None].cuda(), torch.tensor([c["lab"]], dtype=torch.int32).cuda(),
                                     torch.tensor([L], dtype=torch.int32).cuda(), torch.tensor([T], dtype=torch.int32).cuda(),
                                     repeat_from=rf.cuda(), repeat_penalty=0.5)
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert x.tobytes() == y.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ 4. the equal-class rule
def test_a_source_of_the_targets_class_is_passed_over_for_the_second_best():
    """Three lines; line 0 ends in class 7 and line 2 starts with class 7.  Sung: line 0, then line 2 with no breath between them, so the
    best source when line 2 begins is line 0's last label -- the forbidden one.  The restatement must enter line 2 from another source
    (asserted first), and the device must agree."""
    lengths = [4, 4, 4]
    labels = [1, 2, 3, 7, 4, 5, 6, 8, 7, 9, 10, 11]
    c = lo.planted(3, 40, lengths, [0, 2], 3, 0, labels=labels)
    ref = lo.viterbi(c["em"], c["lab"], c["ls"], 0.25)
    path = ref[4]
    t = path.index(2 * 8 + 1)                          # the first frame in line 2's first label
    dp, _, _ = lo.lattice(c["em"], c["lab"], c["ls"], 0.25)
    src, _ = lo.sources(c["lab"], c["ls"])
    best = src[int(np.argmax(dp[t - 1][src]))]
    assert best == 2 * 4 - 1 and c["lab"][best >> 1] == c["lab"][8]                 # the overall best source is the forbidden one
    assert path[t - 1] in src and path[t - 1] != best, (path[t - 1], best)          # ... and the restatement took another
    assert ref.n_jumps >= 1
    _assert_equals_reference(_launch([c], 0.25), 0, ref, c, "equal class")


# ------------------------------------------------------------------------------------------------ 5. invalid inputs (refused by status)
def test_a_clip_without_a_first_line_is_einval_and_its_batch_mates_are_unaffected():
    from lyricalignment_amd import ops
    good, ref = clip_and_reference("two_waves_40x200")
    bad = dict(good, ls=[0] + good["ls"][1:])
    got = _launch([good, bad, good])
    for b in (0, 2):
        _assert_equals_reference(got, b, ref, good, f"clip {b} beside the invalid one")
    assert got[3][1] == lo.LA_EINVAL and got[2][1] == 0.0
    assert (got[0][1] == -1).all() and (got[1][1] == -1).all() and (got[4][1] == -1).all()
    em = torch.from_numpy(good["em"])[None].cuda()
    args = (em, torch.tensor([good["lab"]], dtype=torch.int32).cuda(), torch.tensor([40], dtype=torch.int32).cuda(),
            torch.tensor([200], dtype=torch.int32).cuda(), torch.tensor([good["ls"]], dtype=torch.int32).cuda())
    for pen in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="line_jump_penalty"):
            ops.viterbi_lines_batch(*args, pen)


# ------------------------------------------------------------------------------------------------ 6. the Python surface
@pytest.fixture(scope="module")
def tiny():
    import test_gpu_ragged as tr
    from test_gpu_parity_full import _build
    model, _ = _build("tiny", torch.float32)
    idx = [0, 1, 3, 5]                                           # clips of tests/test_gpu_ragged.py: 11, 5, 8, 3 labels
    return dict(model=model, audios=[tr._clip(i) for i in idx], labels=tr._padded_labels(idx), tr=tr, idx=idx)


LINE_STARTS = [[0, 3, 7, 9], [0, 2], [0, 1, 4], [0]]


def _flags(starts, L):
    return [1 if n in starts else 0 for n in range(L)]


def _expected(em, lists, counts, line_starts, pen):
    """The restatement on a device emission matrix [B, T, >= L+1] (host array) -> (seconds, segments, refs) as the public functions give them."""
    seconds, segments, refs = [], [], []
    for b, labs in enumerate(lists):
        L = len(labs)
        r = lo.viterbi(em[b, : counts[b], : L + 1], labs, _flags(line_starts[b], L), pen)
        assert r[3] == lo.LA_OK
        seconds.append([None if r[0][n] < 0 else [float(r[0][n]) * HOP, float(r[1][n]) * HOP] for n in range(L)])
        segments.append([(n, float(t) * HOP, float(u) * HOP) for n, t, u in lo.segments(r[4])])
        refs.append(r)
    return seconds, segments, refs


@pytest.mark.parametrize("use_ctc", [True, False])
def test_perform_viterbi_and_align_equal_the_restatement_on_the_devices_emissions(tiny, use_ctc):
    from lyricalignment_amd import _lib, ops
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels = tiny["model"], tiny["audios"], tiny["labels"]
    two = ua.perform_viterbi_ctc if use_ctc else ua.perform_viterbi
    variant = _lib.LA_VARIANT_CTC if use_ctc else _lib.LA_VARIANT_PLAIN
    n_jumps = []
    with torch.no_grad():
        logits, _ = model.frame_manual_forward(audios)
        lab, n_lab, lists = ua._labels_to_device(labels, 4, logits.device)
        T = logits.shape[1]
        em = ops.emissions_from_logits(logits.float().contiguous(), lab, n_lab, variant).cpu().numpy()
        eng = model.engine()
        feats, B, T2, stride = model._features(model._mel_of(audios), True)
        em_head = eng.emissions(feats, B, T2, stride, lab, n_lab, variant).cpu().numpy()
        assert T2 == T
        for pen in (0.0, 0.5):
            kw = dict(line_starts=LINE_STARTS, line_jump_penalty=pen)
            seconds, segments, refs = _expected(em, lists, [T] * 4, LINE_STARTS, pen)
            got = two(logits, labels, return_segments=True, **kw)
            assert got[0] == seconds and got[1] == segments, pen
            assert two(logits, labels, **kw) == seconds
            seconds_h, segments_h, refs_h = _expected(em_head, lists, [T] * 4, LINE_STARTS, pen)
            fused = model.align(audios, labels, use_ctc=use_ctc, return_segments=True, **kw)
            assert fused[0] == seconds_h and fused[1] == segments_h, pen
            assert model.align(audios, labels, use_ctc=use_ctc, **kw) == seconds_h
            frames = model.align(audios, labels, use_ctc=use_ctc, return_frames=True, **kw)
            assert len(frames) == 5 and frames[3].tolist() == [0] * 4 and frames[4].dtype == torch.int32
            for b, r in enumerate(refs_h):
                assert frames[4][b].tolist() == r[4] and np.float64(frames[2][b].item()).tobytes() == np.float64(r[2]).tobytes()
            n_jumps.append([r.n_jumps for r in refs_h])
        print(f"use_ctc={use_ctc}: jumps per clip {n_jumps}")
        assert any(n > 0 for row in n_jumps for n in row)
        plain = model.align(audios, labels, use_ctc=use_ctc)
        assert model.align(audios, labels, use_ctc=use_ctc, line_starts=None) == plain          # the call as it was
        assert two(logits, labels, line_starts=None) == two(logits, labels)


def test_per_clip_long_form_readings_and_pronunciation_with_line_starts(tiny):
    from lyricalignment_amd import _lib, ops
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels, tr = tiny["model"], tiny["audios"], tiny["labels"], tiny["tr"]
    kw = dict(line_starts=LINE_STARTS, line_jump_penalty=0.25, return_segments=True)
    with torch.no_grad():
        # per_clip: every clip as if it ran alone, and the restatement on its own frames
        batch = model.align(audios, labels, per_clip=True, **kw)
        logit_rows = model.frame_logits_per_clip(audios)
        for r, i in enumerate(tiny["idx"]):
            alone = model.align([audios[r]], tr._clip_labels(i), per_clip=True, line_starts=[LINE_STARTS[r]], line_jump_penalty=0.25,
                                return_segments=True)
            assert batch[0][r] == alone[0][0] and batch[1][r] == alone[1][0], i
            lg = logit_rows[r][None].float().contiguous()
            lab, n_lab, lists = ua._labels_to_device(tr._clip_labels(i), 1, lg.device)
            em = ops.emissions_from_logits(lg, lab, n_lab, _lib.LA_VARIANT_CTC).cpu().numpy()
            seconds, segments, _ = _expected(em, lists, [lg.shape[1]], [LINE_STARTS[r]], 0.25)
            assert batch[0][r] == seconds[0] and batch[1][r] == segments[0], i
        # the long form: 33 s, two encoder chunks
        audio = np.concatenate([tr._clip(4), tr._clip(3)])
        lab = torch.from_numpy(np.random.RandomState(5).randint(2, 403, size=(1, 14)))
        long_kw = dict(line_starts=[[0, 4, 9]], line_jump_penalty=0.25, return_segments=True)
        logits, _ = model.frame_manual_forward([audio])
        assert logits.shape[1] > 1500
        got = model.align([audio], lab, **long_kw)
        assert got == ua.perform_viterbi_ctc(logits, lab, **long_kw)
        lab_d, n_lab, lists = ua._labels_to_device(lab, 1, logits.device)
        em = ops.emissions_from_logits(logits.float().contiguous(), lab_d, n_lab, _lib.LA_VARIANT_CTC).cpu().numpy()
        seconds, segments, refs = _expected(em, lists, [logits.shape[1]], [[0, 4, 9]], 0.25)
        assert got[0] == seconds and got[1] == segments
        assert refs[0].n_jumps > 0 or refs[0].free_start or refs[0].free_end            # not the plain lattice's path
        # alternatives + return_readings: the lattice sees the per-position ids on the folded matrix; the readings read the first visit
        logits, _ = model.frame_manual_forward(audios)
        alts = [[(1, [17, 23]), (4, [99])], [], [(0, [5])], [(2, [7, 8, 9])]]
        lab_d, n_lab, lists = ua._labels_to_device(labels, 4, logits.device)
        rd = ua._readings_of(alts, lists)
        nf = torch.full((4,), logits.shape[1], dtype=torch.int32, device=logits.device)
        pred = logits.float().contiguous()
        route = ua.readings_route(rd, lambda lab_x, n_x: ops.emissions_from_logits(pred, lab_x, n_x, _lib.LA_VARIANT_CTC), n_lab, nf, logits.device)
        ids = [route.lattice_ids[b, : len(l)].tolist() for b, l in enumerate(lists)]
        seconds, segments, refs = _expected(route.em.cpu().numpy(), ids, [logits.shape[1]] * 4, LINE_STARTS, 0.25)
        got = ua.perform_viterbi_ctc(logits, labels, alternatives=alts, return_readings=True, **kw)
        assert got[0] == seconds and got[1] == segments and len(got) == 3
        fused = model.align(audios, labels, alternatives=alts, return_readings=True, **kw)
        # (the fused head's emissions equal the two-step route's to float32 rounding, not to the bit: the frames agree, the scores nearly)
        assert fused[0] == got[0] and fused[1] == got[1]
        assert [[v and v[0] for v in row] for row in fused[2]] == [[v and v[0] for v in row] for row in got[2]]
        for b, row in enumerate(got[2]):
            assert [v is None for v in row] == [s is None for s in seconds[b]]
        on = torch.tensor([[r[0][n] if n < len(r[0]) else -1 for n in range(labels.shape[1])] for r in refs], dtype=torch.int32).cuda()
        off = torch.tensor([[r[1][n] if n < len(r[1]) else -1 for n in range(labels.shape[1])] for r in refs], dtype=torch.int32).cuda()
        assert got[2] == ua._readings_from_scores(*route.scores(n_lab, on, off), rd)
        # return_pronunciation reads the first visit's boundaries too
        pkw = dict(return_pronunciation=True, pronunciation_classes=40, pronunciation_top_k=3)
        out = model.align(audios, labels, **kw, **pkw)
        two = ua.perform_viterbi_ctc(logits, labels, **kw, **pkw)
        assert len(out) == 3 and out[0] == two[0] and out[1] == two[1]
        assert [[d and (d["class"], d["frames"]) for d in row] for row in out[2]] == [[d and (d["class"], d["frames"]) for d in row] for row in two[2]]
        plain = model.align(audios, labels, **kw)
        assert out[0] == plain[0] and out[1] == plain[1]
        for b, row in enumerate(out[2]):
            for n, d in enumerate(row):
                assert (d is None) == (plain[0][b][n] is None)
                if d is not None:
                    assert d["frames"] == round((plain[0][b][n][1] - plain[0][b][n][0]) / HOP)


def test_align_free_order_on_the_tiny_model(tiny):
    from lyricalignment_amd.harness import PinyinClassLUT, align_free_order
    from test_gpu_parity_full import VOCAB
    model, tr = tiny["model"], tiny["tr"]
    lut = PinyinClassLUT([str(i) for i in range(VOCAB)], {str(i): i for i in range(VOCAB)})           # token id -> the same class id
    ids_all = [int(v) for v in tr._clip_labels(0)[0]]                                                 # 11 labels: lines of 3 / 4 / 2 / 2
    lines = ["".join(chr(0x4E00 + 11 * k + j) for j in range(n)) for k, n in enumerate((3, 4, 2, 2))]
    ids, pos = {}, 0
    for line in lines:
        ids[line] = ids_all[pos: pos + len(line)]
        pos += len(line)
    out = align_free_order(model, tr._clip(0), lines, lut, lambda t: ids[t], line_jump_penalty=0.25)
    with torch.no_grad():
        _, seg = model.align([tr._clip(0)], tr._clip_labels(0), line_starts=[[0, 3, 7, 9]], line_jump_penalty=0.25, return_segments=True)
    starts = [0, 3, 7, 9]
    line_of = [i for i, line in enumerate(lines) for _ in line]
    flat = []
    occ_iter = [iter(o) for o in out["occurrences"]]
    for i in out["order"]:                                          # the occurrences, walked in the reported order, are the visits in time order
        flat += [(c[0], c[1], c[2]) for c in next(occ_iter[i])]
    assert flat == [(a, e, lines[line_of[n]][n - starts[line_of[n]]]) for n, a, e in seg[0]]
    assert out["unsung"] == [i for i in range(4) if i not in out["order"]]
    print(f"order {out['order']}, unsung {out['unsung']}")


# ------------------------------------------------------------------------------------------------ 7. the bench tool
def test_the_bench_tool_runs_quick():
    # --parent-lib: the tree's own library loaded a second time, the control of two loads of one build
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "line_order_bench.py"), "--quick", "--parent-lib",
                        os.path.join(ROOT, "lyricalignment_amd", "liblyricalign_hip.so")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    same = [line for line in r.stdout.splitlines() if "same bits as the parent commit's" in line]
    assert same and all(line.endswith(": yes") for line in same), r.stdout
    assert "viterbi_lines" in r.stdout
