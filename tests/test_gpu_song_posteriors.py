"""Whole-song confidence for repeated lyric lines on the device (la_alignment_posteriors_song: beyond 511 labels the REP face of
posterior_strip_kernel in csrc/la_posterior.hip; ops.alignment_posteriors_song and the layers over it) against the float64 yardstick
tests/repeat_posterior_reference.py, at every number of states per thread (R = 2 / 4 / 8).

Clips: the planted strip shapes of tests/test_gpu_repeat_spans.py, two soft clips per launch (tests/test_gpu_repeat_posteriors.py's
search over OFF_LEVELS), and the sheets of tests/song_posterior_cases.py.  That a case is not vacuous is asserted on the yardstick, never
on the kernel.  Where a clip is built here, onset / offset / path are those of la_viterbi_repeats_batch on the same lattice (pinned bit for
bit by tests/test_gpu_repeat_spans.py): the posteriors are about whatever segments they are handed, and the yardstick gets the same ones.

Tolerance, derived and not tuned: 8 * T * 2**-23 * max(1, yardstick value) on every output, every gamma cell and log_z (the derivation
stands in tests/test_gpu_repeat_posteriors.py)."""
import functools

import numpy as np
import pytest
import torch

import repeat_posterior_reference as rpr
import repeat_spans_reference as rr
import song_posterior_cases as spc
import test_gpu_repeat_posteriors as trp
import test_gpu_repeat_spans as trs
import wide_posterior_cases as wpc
from test_gpu_repeat_posteriors import BW, OFF_LEVELS, soften, tol
from test_gpu_repeat_spans import PEN, RPEN, _plant, make_clip

pytestmark = pytest.mark.gpu

STRIP_GROUPS = ["strip_R2_L512", "strip_R2_L1023", "strip_R4_L1024", "strip_R8_L2048"]
KEYS = ("occupancy", "onset_prob", "offset_prob", "log_z", "status", "visits", "span_skip", "repeat_count", "path_prob", "gamma")


def _pad(width):
    """A clip without frames (status LA_EINVAL) that only makes the label tensors `width` wide: it decides the kernel form."""
    return dict(lab=[1] * width, em=np.zeros((8, width + 1), np.float32), skip=None, rf=None, kind="pad", T=0)


def _run(clips, pen=PEN, rpen=RPEN, windows=None, repeat="own", entry="song", gamma=True, with_path=True, dp=None):
    """One la_viterbi_repeats_batch launch (unless dp = (onset, offset, path) host lists per clip are given) and one launch of the entry
    -> dict of host arrays.  repeat: "own" (the clips' spans; null when none has one), None (null) or "none" (all -1)."""
    from lyricalignment_amd import ops
    d = trp._device(clips, windows)
    rf = {"own": d["rf"], None: None, "none": d["none"]}[repeat]
    if dp is None:
        on, off, _, st_dp, path = ops.viterbi_repeats_batch(*d["base"], d["skip"], pen, *d["win"], rf, rpen)
    else:
        B, Lmax, Tmax = len(clips), d["base"][1].shape[1], d["base"][0].shape[1]
        on_h, off_h = np.full((B, Lmax), -1, np.int32), np.full((B, Lmax), -1, np.int32)
        path_h = np.full((B, Tmax), -1, np.int32)
        for b, (o, f, p) in enumerate(dp):
            on_h[b, : len(o)], off_h[b, : len(f)], path_h[b, : len(p)] = o, f, p
        on, off, path, st_dp = torch.from_numpy(on_h).cuda(), torch.from_numpy(off_h).cuda(), torch.from_numpy(path_h).cuda(), None
    sweep = ops.alignment_posteriors_song if entry == "song" else ops.alignment_posteriors_repeats
    res = sweep(*d["base"], on, off, d["skip"], pen, *d["win"], rf, rpen, path if with_path else None, boundary_window=BW, want_gamma=gamma)
    torch.cuda.synchronize()
    names = KEYS[:9] + (("gamma",) if gamma else ())
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in zip(names, res)}
    out.update(onset=on.cpu().numpy(), offset=off.cpu().numpy(), path=path.cpu().numpy(), dev=d)
    return out


def _dp_of(got, b, c):
    L, T = len(c["lab"]), c.get("T", c["em"].shape[0])
    return got["onset"][b, :L].tolist(), got["offset"][b, :L].tolist(), None, rr.LA_OK, got["path"][b, :T].tolist()


def _report(name, worst):
    print(f"{name}: largest error as a fraction of the bound, and absolute: " + ", ".join(f"{k} {f:.3f} ({e:.2e})" for k, (f, e) in worst.items()))


# ------------------------------------------------------------------------------------------------ 1. every strip form against the yardstick
@functools.lru_cache(maxsize=None)
def soft_clips():
    """The soft clips that ride in every launch, each softened (tests/test_gpu_repeat_posteriors.py's search over OFF_LEVELS) until the
    yardstick says "undecided".  Two are planted at (300, 260), more than one wave of threads at every R: "repeat" (the chorus sung
    twice) until the largest repeat_count lies in [0.1, 0.9], and "both" until the count is fractional and span_skip > 0.1.  The
    "declared" clip (sung straight through) is the (100, 33) clip of that module's wide groups: at 260 labels in 300 frames a second
    pass of the chorus has no frames to spare and the yardstick's count never reaches 0.1 at any level (0.016 at most over 60 seeds and
    frame counts up to 520), so the search cannot end there."""
    out = []
    for kind, T, L in (("declared", 100, 33), ("repeat", 300, 260), ("both", 300, 260)):
        base = make_clip(sum(map(ord, "16_waves_L511")) + 3 if kind == "declared" else 2031, T, L, kind)
        chosen = None
        for off in OFF_LEVELS:
            c = soften(base, off)
            ref = rpr.posteriors(c["em"], c["lab"], c["skip"], PEN, c["rf"], RPEN)
            x = float(ref["repeat_count"].max())
            if 0.1 <= x <= 0.9 if kind != "both" else (abs(x - round(x)) > 0.05 and ref["span_skip"].max() > 0.1):
                chosen = c
                break
        assert chosen is not None, kind
        r = trs.reference(chosen)
        assert r[3] == rr.LA_OK
        out.append((chosen, r, trp.yardstick(chosen, r)))
    return out


@functools.lru_cache(maxsize=None)
def strip_cases(name):
    clips, refs = trs.reference_cases(name)
    clips, refs = list(clips), list(refs)
    ys = [trp.yardstick(c, r) for c, r in zip(clips, refs)]
    for c, r, y in soft_clips():
        clips.append(c); refs.append(r); ys.append(y)
    return clips, refs, ys


@pytest.mark.parametrize("name", STRIP_GROUPS)
def test_every_strip_form_equals_the_float64_yardstick(name):
    clips, refs, ys = strip_cases(name)
    rc = [float(y["repeat_count"].max()) for y in ys]
    assert any(x > 0.9 for x in rc) and any(c["rf"] is not None and x < 0.1 for c, x in zip(clips, rc)), name
    assert 0.1 <= rc[-3] <= 0.9 and 0.1 <= rc[-2] <= 0.9 and abs(rc[-1] - round(rc[-1])) > 0.05 and ys[-1]["span_skip"].max() > 0.1, (name, rc)
    assert clips[-3]["kind"] == "soft declared" and len(clips[-2]["lab"]) == len(clips[-1]["lab"]) == 260
    got = _run(clips)
    worst = {}
    for b, (c, r, y) in enumerate(zip(clips, refs, ys)):
        L = len(c["lab"])
        assert got["onset"][b, :L].tolist() == r[0] and got["offset"][b, :L].tolist() == r[1] and got["path"][b, : len(r[4])].tolist() == r[4]
        trp._assert_close(got, b, c, y, (name, b, c["kind"]), worst)
        trp._assert_identity(got, b, c, (name, b, c["kind"]))
    print(f"{name}: repeat_count maxima per clip {[round(x, 3) for x in rc]}; largest visits {max(float(y['visits'].max()) for y in ys):.3f}")
    _report(name, worst)


# ------------------------------------------------------------------------------------------------ 2. 4095 labels, the top threads
def test_4095_labels_with_the_chorus_in_the_last_200_labels():
    """The repeated chorus lies in labels 3900 .. 4089: its states belong to the last threads of the workgroup at R = 8.  log_z against
    a forward-only float64 sweep (the full yardstick is too large here: this sweep takes a few seconds), and the visit identity on the
    device's own outputs."""
    L, a, e = 4095, 3900, 4090
    T = L + (e - a) + 125                       # just above what the planting needs: every sung label a frame, the breaths, some silence
    rs = np.random.RandomState(4095)
    lab = trs._labels(4095, L)
    sung = list(range(0, e)) + list(range(a, e)) + list(range(e, L))
    rf = [-1] * L
    rf[a] = e
    c = soften(dict(lab=lab, em=_plant(rs, T, L, sung, spc.breaths_of(lab, sung)), skip=None, rf=rf, kind="top"), -3.0)
    want = spc.forward_log_z(c["em"], lab, None, 0.0, rf, RPEN)
    without = spc.forward_log_z(c["em"], lab, None, 0.0, None, 0.0)
    assert np.isfinite(want) and want - without > 100.0        # on the yardstick: nearly all the mass returns through the repeat arcs
    got = _run([c], gamma=False)
    assert got["status"][0] == rr.LA_OK
    err = abs(float(got["log_z"][0]) - want)
    print(f"4095 labels, T = {T}: log_z {float(got['log_z'][0])!r} against {want!r}: {err:.3e}, bound {float(tol(T, abs(want))):.3e}")
    assert err <= tol(T, abs(want))
    trp._assert_identity(got, 0, c, "4095 labels")
    assert got["repeat_count"][0, a] > 0.9 and not np.delete(got["repeat_count"][0], a).any()
    path = got["path"][0, :T]
    assert (got["path_prob"][0, :T] > 0).all() and path.max() >= 2 * L - 1 and path.min() >= 0 and not got["path_prob"][0, T:].any()


# ------------------------------------------------------------------------------------------------ 3. long, mixed arc lists
@functools.lru_cache(maxsize=None)
def mixed_case(L):
    """song_posterior_cases.mixed_sheet planted and softened until the yardstick gives both spans that share the end 101 a repeat_count of
    at least 0.05 -> clip, yardstick posteriors (without the scores: they need the DP's segments)."""
    skip, rf, sung = spc.mixed_sheet(L)
    lab = wpc.labels_of(L, L)
    breaths = spc.breaths_of(lab, sung)
    T = len(sung) + len(breaths) + 30
    base = dict(lab=lab, em=_plant(np.random.RandomState(L), T, L, sung, breaths), skip=skip, rf=rf, kind="mixed")
    for off in OFF_LEVELS:
        c = soften(base, off)
        ref = rpr.posteriors(c["em"], lab, skip, PEN, rf, RPEN)
        if min(ref["repeat_count"][95], ref["repeat_count"][97]) >= 0.05 and abs(ref["repeat_count"][95] - 1.0) > 1e-3:
            return c, ref
    raise AssertionError(L)


def _yardstick_of(c, ref, dp):
    occ, onp, offp = rpr.scores(ref, dp[0], dp[1], BW)
    return dict(occupancy=occ, onset_prob=onp, offset_prob=offp, visits=ref["visits"], span_skip=ref["span_skip"],
                repeat_count=ref["repeat_count"], path_prob=rpr.path_prob(ref, dp[4]), gamma=ref["gamma"], log_z=ref["log_z"])


@pytest.mark.parametrize("L", [512, 1024, 2048])
def test_long_arc_lists_with_skip_words_followed_by_repeat_words(L):
    c, ref = mixed_case(L)
    R = wpc.strip_states_per_thread(L)
    longest = spc.assert_mixed_arc_lists(c["skip"], c["rf"], c["lab"], R)
    rc = ref["repeat_count"]
    assert rc[95] >= 0.05 and rc[97] >= 0.05 and rc[103] >= 0.05 and rc[104] >= 0.05, rc[[95, 97, 103, 104]]
    got = _run([c])
    dp = _dp_of(got, 0, c)
    worst = {}
    trp._assert_close(got, 0, c, _yardstick_of(c, ref, dp), ("mixed", L), worst)
    trp._assert_identity(got, 0, c, ("mixed", L))
    print(f"L = {L}, R = {R}: longest arc list {longest} words; repeat_count of the four spans {[round(float(rc[a]), 3) for a in (95, 97, 103, 104)]}")
    _report(f"mixed L = {L}", worst)


# ------------------------------------------------------------------------------------------------ 4. the same bits in both kernels
def test_a_clip_gives_the_same_bits_in_the_lane_form_and_in_every_strip_form():
    clips = [make_clip(41, 40, 5, "both"), soften(make_clip(42, 340, 300, "both"), -2.0), soften(make_clip(43, 560, 511, "repeat"), -2.0),
             make_clip(44, 330, 300, "declared")]
    assert any(c["skip"] is not None for c in clips) and all(c["rf"] is not None for c in clips)
    y = rpr.posteriors(clips[1]["em"], clips[1]["lab"], clips[1]["skip"], PEN, clips[1]["rf"], RPEN)
    assert y["repeat_count"].max() > 0.1 and y["span_skip"].max() > 0.1                  # on the yardstick: both kinds of arc carry mass
    lane = _run(clips, entry="repeats")
    assert (lane["status"] == rr.LA_OK).all()
    dp = [_dp_of(lane, b, c) for b, c in enumerate(clips)]
    same = _run(clips, entry="song")                       # up to 511 labels the new entry IS the older entry's sweep
    for k in KEYS:
        assert same[k].tobytes() == lane[k].tobytes(), k
    for width in (512, 1024, 2048):
        wide = _run(clips + [_pad(width)], entry="song", dp=[(r[0], r[1], r[4]) for r in dp] + [([], [], [])])
        assert wide["status"].tolist() == [rr.LA_OK] * len(clips) + [rr.LA_EINVAL]
        for b, c in enumerate(clips):
            va, vb = trp._clip_view(wide, b, c), trp._clip_view(lane, b, c)
            for k in va:
                assert np.asarray(va[k]).tobytes() == np.asarray(vb[k]).tobytes(), (width, b, k)
            L, T = len(c["lab"]), c["em"].shape[0]
            assert not wide["repeat_count"][b, L:].any() and not wide["path_prob"][b, T:].any() and not wide["gamma"][b, T:].any()


# ------------------------------------------------------------------------------------------------ 5. nothing repeatable
@pytest.mark.parametrize("T,L", [(560, 512), (1100, 1024), (2200, 2048)])
def test_null_and_all_minus_one_repeat_from_equal_the_lattice_entry_bit_for_bit(T, L):
    from lyricalignment_amd import ops
    for v, name in enumerate(wpc.LATTICES):
        case = wpc.lattice_case(T, L, v)
        c = dict(lab=case["lab"], em=np.array(case["em"]), skip=case["skip"], rf=None, kind=name)
        wins = None if case["lo"] is None else [(case["lo"], case["hi"])]
        dp = [(case["on"], case["off"], [])]
        a, b = _run([c], pen=case["pen"], windows=wins, repeat=None, dp=dp), _run([c], pen=case["pen"], windows=wins, repeat="none", dp=dp)
        d = a["dev"]
        on, off = torch.from_numpy(a["onset"]).cuda(), torch.from_numpy(a["offset"]).cuda()
        want = ops.alignment_posteriors_lattice(*d["base"], on, off, d["skip"], case["pen"], *d["win"], boundary_window=BW, want_gamma=True)
        want = dict(zip(("occupancy", "onset_prob", "offset_prob", "log_z", "status", "visits", "span_skip", "gamma"), (t.cpu().numpy() for t in want)))
        assert (want["status"] == rr.LA_OK).all() and want["occupancy"].any(), name
        for got in (a, b):
            for k, w in want.items():
                assert got[k].tobytes() == w.tobytes(), (T, L, name, k)          # visits = present_prob
            assert not got["repeat_count"].any() and not got["path_prob"].any(), (T, L, name)      # (the path given names no state)
        if case["skip"] is not None:
            assert (want["span_skip"] > 0.0).any() and (want["visits"] < 1.0).any()


# ------------------------------------------------------------------------------------------------ 6. windows
def test_windows_with_a_taken_repeat_arc():
    """The mixed sheet at 512 labels with two windows that bind: label 300's state may be held only in four frames that begin two frames
    after the planting has sung it, and the last label not before its planted segment.  Against the yardstick with the same windows."""
    c, open_ref = mixed_case(512)
    L, T = 512, c["em"].shape[0]
    S = 2 * L + 1
    truth = [int(np.argmax(row)) for row in c["em"]]          # softening keeps the sung cell the largest of its row
    frames = [t for t, col in enumerate(truth) if col == 301]
    lo, hi = [0] * S, [T] * S
    lo[601], hi[601] = frames[-1] + 2, frames[-1] + 6
    last = [t for t, col in enumerate(truth) if col == L]
    lo[2 * L - 1] = last[0]
    ref = rpr.posteriors(c["em"], c["lab"], c["skip"], PEN, c["rf"], RPEN, lo, hi)
    assert np.isfinite(ref["log_z"]) and ref["repeat_count"][[95, 97]].min() >= 0.05
    assert np.abs(ref["gamma"] - open_ref["gamma"]).max() > 1e-3 and ref["log_z"] < open_ref["log_z"] - 1e-3       # the windows bind
    got = _run([c], windows=[(lo, hi)])
    worst = {}
    trp._assert_close(got, 0, c, _yardstick_of(c, ref, _dp_of(got, 0, c)), "windows", worst)
    trp._assert_identity(got, 0, c, "windows")
    assert not got["gamma"][0, : lo[601], 601].any() and not got["gamma"][0, hi[601]: T, 601].any()
    _report("windows", worst)


# ------------------------------------------------------------------------------------------------ 7. edges
def test_one_to_seven_frames_infeasible_clips_no_path_batch_mates_and_two_calls():
    """T = 1 .. 7 on the strip kernel with a declared repeat span: the prefetch tails meet the first-frame and last-frame branches; three
    labels in one or two frames is LA_EINFEASIBLE with every row zeroed."""
    lab, rf, skip = [3, 5, 3], [2, -1, -1], [-1, -1, 1, -1]
    rs = np.random.RandomState(7)
    clips = [dict(lab=lab, em=np.log(rs.dirichlet(np.ones(4), size=T)).astype(np.float32), skip=skip, rf=rf, kind=f"T={T}") for T in range(1, 8)]
    clips.append(dict(make_clip(9, 60, 20, "repeat"), T=7))                 # 20 labels in 7 frames
    refs = [rr.viterbi(c["em"][: c.get("T", len(c["em"]))], c["lab"], c["skip"], PEN, c["rf"], RPEN, rows=True) for c in clips]
    want_status = [rr.LA_EINFEASIBLE, rr.LA_EINFEASIBLE] + [rr.LA_OK] * 5 + [rr.LA_EINFEASIBLE]
    assert [r[3] for r in refs] == want_status
    ys = [trp.yardstick(c, r) if r[3] == rr.LA_OK else None for c, r in zip(clips, refs)]
    assert max(float(y["repeat_count"].max()) for y in ys if y is not None) > 0.01        # the declared arc carries mass somewhere
    batch = clips + [_pad(512)]
    first, second = _run(batch), _run(batch)
    assert first["status"].tolist() == want_status + [rr.LA_EINVAL]
    for k in KEYS:
        assert first[k].tobytes() == second[k].tobytes(), k                  # two calls agree to the bit
    for b, (c, r, y) in enumerate(zip(clips, refs, ys)):
        if y is None:
            assert np.isneginf(first["log_z"][b])
            for k in ("occupancy", "onset_prob", "offset_prob", "visits", "span_skip", "repeat_count", "path_prob", "gamma"):
                assert not first[k][b].any(), (b, k)
            continue
        assert first["onset"][b, :3].tolist() == r[0] and first["path"][b, : len(r[4])].tolist() == r[4]
        trp._assert_close(first, b, c, y, c["kind"])
        trp._assert_identity(first, b, c, c["kind"])
    for k in ("occupancy", "onset_prob", "offset_prob", "visits", "span_skip", "repeat_count", "path_prob", "gamma"):
        assert not first[k][len(clips)].any(), k                             # the clip without frames
    no_path = _run(batch, with_path=False)
    assert no_path["path_prob"] is None
    for k in KEYS:
        if k != "path_prob":
            assert no_path[k].tobytes() == first[k].tobytes(), k
    alone = _run([clips[6], _pad(512)])                                      # T = 7 alone against T = 7 among its batch mates
    va, vb = trp._clip_view(alone, 0, clips[6]), trp._clip_view(first, 6, clips[6])
    for k in va:
        assert np.asarray(va[k]).tobytes() == np.asarray(vb[k]).tobytes(), k


# ------------------------------------------------------------------------------------------------ 8. the Python surface
tiny = trs.tiny            # the tiny random-weight model and clips of tests/test_gpu_repeat_spans.py


def test_perform_viterbi_ctc_song_scored_gives_the_ops_numbers():
    from lyricalignment_amd import _lib, ops
    from lyricalignment_amd.utils import alignment as ua
    rs = np.random.RandomState(600)
    T, L, V = 700, 600, 64
    logits = torch.from_numpy(rs.randn(1, T, V).astype(np.float32) * 3.0).cuda()
    labels = torch.from_numpy(rs.randint(2, V - 1, size=(1, L)))
    kw = dict(repeat_spans=[[(580, 590)]], optional_spans=[[(100, 110)]], skip_penalty=0.5, repeat_penalty=0.25)
    seconds, segments, scores = ua.perform_viterbi_ctc_song_scored(logits, labels, return_segments=True, **kw)
    assert (seconds, scores) == ua.perform_viterbi_ctc_song_scored(logits, labels, **kw)
    with pytest.raises(NotImplementedError):
        ua.perform_viterbi_ctc_repeat_scored(logits, labels, **kw)           # the older function keeps its limit
    lab, n_lab, lists = ua._labels_to_device(labels, 1, logits.device)
    em = ops.emissions_from_logits(logits, lab, n_lab, _lib.LA_VARIANT_CTC)
    nf = torch.full((1,), T, dtype=torch.int32, device=logits.device)
    skip = ua._skip_from_of_spans(kw["optional_spans"], lists).cuda()
    rf = ua._repeat_from_of_spans(kw["repeat_spans"], lists).cuda()
    on, off, score, st, path = ops.viterbi_repeats_batch(em, lab, n_lab, nf, skip, 0.5, None, None, rf, 0.25)
    occ, onp, offp, log_z, status, visits, span_skip, rc, pp = ops.alignment_posteriors_song(em, lab, n_lab, nf, on, off, skip, 0.5, None, None,
                                                                                             rf, 0.25, path, boundary_window=2)
    d = scores[0]
    assert int(status[0]) == rr.LA_OK and set(d) == {"occupancy", "onset_prob", "offset_prob", "path_log_posterior", "visits", "repeat_count",
                                                     "span_skip_prob", "visit_occupancy"}
    assert d["occupancy"] == occ[0].tolist() and d["onset_prob"] == onp[0].tolist() and d["offset_prob"] == offp[0].tolist()
    assert d["visits"] == visits[0].tolist() and d["repeat_count"] == {(580, 590): float(rc[0, 580])}
    assert d["span_skip_prob"] == [float(span_skip[0, 110])] and d["path_log_posterior"] == float(score[0] - log_z[0])
    assert len(d["visit_occupancy"]) == len(segments[0]) and [s for s in seconds[0] if s is not None]
    r = ua.run_lattice(em, lab, n_lab, nf, skip.cpu(), None, 0.5, "song", 2, repeat_from=rf.cpu(), repeat_penalty=0.25)
    assert torch.equal(r.repeat_count, rc) and torch.equal(r.path_prob, pp) and torch.equal(r.visits, visits) and r.log_z_free is None


def test_up_to_511_labels_the_song_keyword_is_the_repeat_keyword(tiny):
    model, audios, labels = tiny["model"], tiny["audios"], tiny["labels"]
    anchors = [[(4, 1.0, 0.5)], [], [], []]
    with torch.no_grad():
        for kw in (dict(repeat_spans=trs.REPEATS), dict(repeat_spans=trs.REPEATS, optional_spans=trs.OPTIONAL, skip_penalty=0.5, onset_anchors=anchors),
                   dict(repeat_spans=trs.REPEATS, per_clip=True)):
            assert model.align(audios, labels, return_segments=True, return_song_confidence=True, **kw) == \
                model.align(audios, labels, return_segments=True, return_repeat_confidence=True, **kw)
            assert model.align(audios, labels, return_song_confidence=True, **kw) == model.align(audios, labels, return_repeat_confidence=True, **kw)
        for other in ("return_confidence", "return_span_confidence", "return_anchored_confidence", "return_sheet_confidence",
                      "return_repeat_confidence"):
            with pytest.raises(ValueError):
                model.align(audios, labels, return_song_confidence=True, **{other: True})


def test_a_sheet_of_more_than_511_characters_with_a_repeatable_line(tiny):
    from lyricalignment_amd.harness import PinyinClassLUT, align_song
    from lyricalignment_amd.utils import alignment as ua
    from test_gpu_parity_full import VOCAB
    model, tr = tiny["model"], tiny["tr"]
    audio = np.concatenate([tr._clip(4), tr._clip(3)])                                     # 33 s: more than 1500 frames, two encoder chunks
    n_lines, per = 52, 10                                                                  # 520 characters
    ids_all = np.random.RandomState(52).randint(2, 403, size=n_lines * per).tolist()
    lines = ["".join(chr(0x4E00 + per * k + j) for j in range(per)) for k in range(n_lines)]
    ids = {line: ids_all[per * k: per * (k + 1)] for k, line in enumerate(lines)}
    labels = torch.tensor([ids_all], dtype=torch.int64)
    repeatable = [k == 20 for k in range(n_lines)]
    optional = [k == 30 for k in range(n_lines)]
    kw = dict(repeat_spans=[[(200, 210)]], optional_spans=[[(300, 310)]])
    with torch.no_grad():
        with pytest.raises(NotImplementedError):
            model.align([audio], labels, return_repeat_confidence=True, **kw)
        seconds, segments, scores = model.align([audio], labels, return_song_confidence=True, return_segments=True, **kw)
        logits, _ = model.frame_manual_forward([audio])
        steps = ua.perform_viterbi_ctc_song_scored(logits, labels, return_segments=True, **kw)
    assert (seconds, segments) == steps[:2]
    trp._scores_close(scores[0], steps[2][0], logits.shape[1], "520 characters")
    trp._check_scores(seconds, segments, scores, kw["repeat_spans"], kw["optional_spans"], False)
    lut = PinyinClassLUT([str(i) for i in range(VOCAB)], {str(i): i for i in range(VOCAB)})           # token id -> the same class id
    occ, conf = align_song(model, audio, lines, lut, lambda t: ids[t], optional=optional, repeatable=repeatable)
    assert set(conf) == {"sung", "line_onset_prob", "window_log_prob", "visits", "repeat_count", "occurrence_occupancy"}
    assert len(occ) == n_lines and all(len(conf[k]) == n_lines for k in ("sung", "line_onset_prob", "visits", "repeat_count", "occurrence_occupancy"))
    d = scores[0]
    assert conf["visits"] == [d["visits"][per * k] for k in range(n_lines)] and conf["window_log_prob"] == 0.0
    assert conf["repeat_count"] == [d["repeat_count"][(200, 210)] if k == 20 else None for k in range(n_lines)]
    assert conf["sung"][20] == d["visits"][200] - d["repeat_count"][(200, 210)] and conf["sung"][3] == d["visits"][30]
    for k in range(n_lines):
        assert len(conf["occurrence_occupancy"][k]) == len(occ[k])
        assert (conf["line_onset_prob"][k] is None) == (seconds[0][per * k] is None) == (len(occ[k]) == 0)
        for o in occ[k]:
            assert [ch for _, _, ch in o] == list(lines[k])[: len(o)] or len(o) <= per
    plain, old = align_song(model, audio, lines, lut, lambda t: ids[t], optional=optional)            # without repeatable: unchanged
    assert set(old) == {"sung", "line_onset_prob", "window_log_prob"} and len(plain) == n_lines
    print(f"520 characters: visits of the repeatable line {conf['visits'][20]:.3f}, returns {conf['repeat_count'][20]:.3f}, occurrences {len(occ[20])}")
