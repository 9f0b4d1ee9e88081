"""Confidence for repeated lyric lines on the device (la_alignment_posteriors_repeats: the REP face of posterior_kernel in
csrc/la_posterior.hip; ops.alignment_posteriors_repeats) against the float64 yardstick tests/repeat_posterior_reference.py (pinned by
tests/test_host_repeat_posteriors.py against path enumeration), in every kernel form.

Clips: the planted clips of tests/test_gpu_repeat_spans.py (make_clip, imported) plus a SOFT family -- the same planting with the
off-path level raised from -6 towards the sung level, per shape until the yardstick's repeat_count lies strictly inside (0, 1) -- because
on the hard clips every count is 0 or 1 to many digits.  That a shape is not vacuous is asserted on the yardstick, never on the kernel.

Tolerance, derived and not tuned: 8 * T * 2**-23 * max(1, yardstick value) on every output, every gamma cell and log_z.  8 T 2^-23 is the
bound of tests/test_gpu_span_posteriors.py (T steps of alpha and of beta with a float32 log-sum-exp correction of <= ~2^-23 each, gamma
adds the two, a two-fold margin for hardware exp / log): it bounds the RELATIVE error of every term exp(alpha + beta - log_z), and on this
lattice visits, onset_prob, offset_prob, repeat_count and span_skip_prob are expected counts -- sums of such terms that exceed 1 -- whose
absolute error grows with their value."""
import functools

import numpy as np
import pytest
import torch

import repeat_posterior_reference as rpr
import repeat_spans_reference as rr
import test_gpu_repeat_spans as trs
from test_gpu_repeat_spans import PEN, RPEN, make_clip

pytestmark = pytest.mark.gpu

BW = 2
GROUPS = ["one_wave_dpp", "one_wave_lds", "2_waves_L33", "4_waves_L100", "8_waves_L200", "16_waves_L511"]
# the clip a group's soft clips are planted on (small: they ride in the group's launch, whose form max_labels decides)
SOFT_SHAPE = {"one_wave_dpp": (64, 12), "one_wave_lds": (64, 12), "2_waves_L33": (50, 9), "4_waves_L100": (90, 40), "8_waves_L200": (100, 33),
              "16_waves_L511": (100, 33)}
OFF_LEVELS = tuple(-3.0 + 0.125 * i for i in range(22))   # -3 .. -0.375 in dyadic steps
OUTS = ("occupancy", "onset_prob", "offset_prob", "visits", "span_skip", "repeat_count", "path_prob", "gamma", "log_z")


def tol(T, ref):
    return 8 * T * 2.0 ** -23 * np.maximum(1.0, ref)


def soften(c, off):
    """The clip with its off-path cells (-6 minus dyadic noise) raised so that -6 becomes `off`; the sung cells stay -0.25."""
    em = np.where(c["em"] == np.float32(-0.25), c["em"], c["em"] + np.float32(6.0 + off)).astype(np.float32)
    return dict(c, em=np.ascontiguousarray(em), kind="soft " + c["kind"], off=off)


def yardstick(c, r, pen=PEN, rpen=RPEN, lo=None, hi=None, rf="own"):
    """-> dict of the entry's outputs as float64 for clip c and the DP result r (onset, offset, score, status, path)."""
    T = c.get("T", c["em"].shape[0])
    ref = rpr.posteriors(c["em"][:T], c["lab"], c["skip"], pen, c["rf"] if rf == "own" else rf, rpen, lo, hi)
    occ, onp, offp = rpr.scores(ref, r[0], r[1], BW)
    return dict(occupancy=occ, onset_prob=onp, offset_prob=offp, visits=ref["visits"], span_skip=ref["span_skip"],
                repeat_count=ref["repeat_count"], path_prob=rpr.path_prob(ref, r[4]), gamma=ref["gamma"], log_z=ref["log_z"])


@functools.lru_cache(maxsize=None)
def cases(name):
    """-> clips, DP references, yardsticks of one shape group: the hard clips of test_gpu_repeat_spans plus two soft ones."""
    clips, refs = trs.reference_cases(name)
    clips, refs = list(clips), list(refs)
    T, L = SOFT_SHAPE[name]
    seed = sum(map(ord, name))
    for kind in ("declared", "both"):
        base = make_clip(seed + (5 if kind == "both" else 3), T, L, kind)
        chosen = None
        for off in OFF_LEVELS:                       # adjusted per shape until the yardstick says "undecided"
            c = soften(base, off)
            r = trs.reference(c)
            if r[3] != rr.LA_OK:
                continue
            y = yardstick(c, r)
            x = float(y["repeat_count"].max())
            # sung straight through: undecided; sung twice with a line left out: fractional (counts between 1 and 2 occur), the skip too
            if 0.1 <= x <= 0.9 if kind == "declared" else (abs(x - round(x)) > 0.05 and y["span_skip"].max() > 0.1):
                chosen = (c, r)
                break
        assert chosen is not None, (name, kind)
        clips.append(chosen[0]); refs.append(chosen[1])
    return clips, refs, [yardstick(c, r) for c, r in zip(clips, refs)]


# ------------------------------------------------------------------------------------------------ launch
def _device(clips, windows=None, Tmax=None):
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
    any_rf = any(c["rf"] is not None for c in clips)
    return dict(base=(em.cuda(), labels.cuda(), n_labels.cuda(), n_frames.cuda()), skip=skip.cuda() if any_skip else None,
                win=(lo.cuda(), hi.cuda()) if windows is not None else (None, None), rf=rf.cuda() if any_rf else None,
                none=torch.full((B, Lmax), -1, dtype=torch.int32).cuda())


def _run(clips, pen=PEN, rpen=RPEN, windows=None, repeat="own", dp_repeat=None, gamma=True):
    """One la_viterbi_repeats_batch launch (its onset / offset / path are the posteriors' inputs) and one la_alignment_posteriors_repeats
    launch -> dict of host arrays.  repeat: "own" (the clips' spans; null when none has one), None (null) or "none" (all -1)."""
    from lyricalignment_amd import ops
    d = _device(clips, windows)
    rf = {"own": d["rf"], None: None, "none": d["none"]}[repeat]
    dp_rf = rf if dp_repeat is None else {"own": d["rf"], "null": None}[dp_repeat]
    on, off, score, st_dp, path = ops.viterbi_repeats_batch(*d["base"], d["skip"], pen, *d["win"], dp_rf, rpen if dp_repeat is None else RPEN)
    res = ops.alignment_posteriors_repeats(*d["base"], on, off, d["skip"], pen, *d["win"], rf, rpen, path, boundary_window=BW, want_gamma=gamma)
    torch.cuda.synchronize()
    names = ("occupancy", "onset_prob", "offset_prob", "log_z", "status", "visits", "span_skip", "repeat_count", "path_prob") + (("gamma",) if gamma else ())
    out = {k: v.cpu().numpy() for k, v in zip(names, res)}
    out.update(onset=on.cpu().numpy(), offset=off.cpu().numpy(), path=path.cpu().numpy(), dp_status=st_dp.cpu().numpy(), dev=d)
    return out


def _clip_view(got, b, c):
    """The rows of clip b cut to its own L / T."""
    L, T = len(c["lab"]), c.get("T", c["em"].shape[0])
    v = {k: got[k][b, :L] for k in ("occupancy", "onset_prob", "offset_prob", "visits", "repeat_count")}
    v.update(span_skip=got["span_skip"][b, : L + 1], path_prob=got["path_prob"][b, :T], log_z=got["log_z"][b])
    if "gamma" in got:
        v["gamma"] = got["gamma"][b, :T, : 2 * L + 1]
    return v


def _assert_close(got, b, c, y, what, worst=None):
    L, T = len(c["lab"]), c.get("T", c["em"].shape[0])
    v = _clip_view(got, b, c)
    assert got["status"][b] == rr.LA_OK, what
    for k in OUTS:
        if k not in v:
            continue
        g, w = np.asarray(v[k], np.float64), np.asarray(y[k], np.float64)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        err = np.abs(g - w)
        frac = float(np.max(err / tol(T, w))) if err.size else 0.0
        if worst is not None:
            worst[k] = max(worst.get(k, (0.0, 0.0)), (frac, float(err.max()) if err.size else 0.0))
        assert frac <= 1.0, (what, k, float(err.max()), frac)
    # what lies past the clip's own L / T is zero
    for k in ("occupancy", "onset_prob", "offset_prob", "visits", "repeat_count"):
        assert not got[k][b, L:].any(), (what, k)
    assert not got["span_skip"][b, L + 1:].any() and not got["path_prob"][b, T:].any(), what
    if "gamma" in got:
        assert not got["gamma"][b, T:].any() and not got["gamma"][b, :, 2 * L + 1:].any(), what


def _assert_identity(got, b, c, what):
    """visits[n] + the skip mass over n = 1 + the return mass over n, on the DEVICE outputs; each term within its own bound."""
    T = c.get("T", c["em"].shape[0])
    v = {k: np.asarray(x, np.float64) for k, x in _clip_view(got, b, c).items() if k in ("visits", "span_skip", "repeat_count")}
    left, right = rpr.identity_sides(v["visits"], v["span_skip"], v["repeat_count"], c["skip"], c["rf"])
    bound = tol(T, v["visits"])
    for a, n in rpr.skip_spans_of(c["skip"]):
        bound[a:n] += tol(T, v["span_skip"][n])
    for a, e in rpr.repeat_spans_of(c["rf"], len(c["lab"])):
        bound[a:e] += tol(T, v["repeat_count"][a])
    assert (np.abs(left - right) <= bound).all(), (what, float(np.abs(left - right).max()))


# ------------------------------------------------------------------------------------------------ 1. accuracy, every form
@pytest.mark.parametrize("name", GROUPS)
def test_equals_the_float64_yardstick_in_every_form(name):
    from lyricalignment_amd import _lib
    clips, refs, ys = cases(name)
    rc = [float(y["repeat_count"].max()) if len(c["lab"]) else 0.0 for c, y in zip(clips, ys)]
    assert any(x > 0.9 for x in rc), name                                                         # the chorus certainly came back
    assert any(c["rf"] is not None and x < 0.1 for c, x in zip(clips, rc)), name                  # arcs declared, certainly not taken
    assert any(c["kind"].startswith("soft") and 0.1 <= x <= 0.9 for c, x in zip(clips, rc)), name  # undecided
    assert any(c["skip"] is not None and y["span_skip"].max() > 0.1 and x > 0.1 for c, y, x in zip(clips, ys, rc)), name
    with _lib.option("viterbi_dpp", 0 if name == "one_wave_lds" else 1):
        got = _run(clips)
    worst = {}
    for b, (c, r, y) in enumerate(zip(clips, refs, ys)):
        L = len(c["lab"])
        assert got["onset"][b, :L].tolist() == r[0] and got["offset"][b, :L].tolist() == r[1] and got["path"][b, : len(r[4])].tolist() == r[4]
        _assert_close(got, b, c, y, (name, b, c["kind"]), worst)
        _assert_identity(got, b, c, (name, b, c["kind"]))
        assert abs(float(got["gamma"][b, : c["em"].shape[0]].sum(1).max()) - 1.0) < 1e-3
    print(f"{name}: repeat_count maxima per clip {[round(x, 3) for x in rc]}; largest visits {max(float(y['visits'].max()) for y in ys):.3f}")
    print(f"{name}: largest error as a fraction of the bound, and absolute: " + ", ".join(f"{k} {f:.3f} ({e:.2e})" for k, (f, e) in worst.items()))


# ------------------------------------------------------------------------------------------------ 2. nothing repeatable = the lattice entry
@pytest.mark.parametrize("name", GROUPS)
def test_null_and_all_minus_one_repeat_from_equal_the_lattice_entry_bit_for_bit(name):
    from lyricalignment_amd import _lib, ops
    clips, refs, _ = cases(name)
    rs = np.random.RandomState(len(name))
    with _lib.option("viterbi_dpp", 0 if name == "one_wave_lds" else 1):
        for face in ("nothing", "spans", "spans + windows", "windows"):
            these = [dict(c, skip=None) for c in clips] if face in ("nothing", "windows") else clips
            wins = None
            if "windows" in face:                     # around each clip's own repeat-free path, widened at random: they bind somewhere
                free = [rr.viterbi(c["em"], c["lab"], c["skip"], PEN, None, 0.0, rows=True) for c in these]
                wins = [trs._windows_around(rs, r[4], 2 * len(c["lab"]) + 1, c["em"].shape[0]) for c, r in zip(these, free)]
            a, b = _run(these, windows=wins, repeat=None), _run(these, windows=wins, repeat="none")
            d = a["dev"]
            on, off = torch.from_numpy(a["onset"]).cuda(), torch.from_numpy(a["offset"]).cuda()
            want = ops.alignment_posteriors_lattice(*d["base"], on, off, d["skip"], PEN, *d["win"], boundary_window=BW, want_gamma=True)
            want = dict(zip(("occupancy", "onset_prob", "offset_prob", "log_z", "status", "visits", "span_skip", "gamma"), (t.cpu().numpy() for t in want)))
            assert (want["status"] == rr.LA_OK).all(), face
            for got in (a, b):
                for k, w in want.items():
                    assert got[k].tobytes() == w.tobytes(), (name, face, k)          # visits = present_prob
                assert not got["repeat_count"].any(), (name, face)
            if face == "spans":
                assert (want["span_skip"] > 0.5).any() and (want["visits"] < 0.5).any()      # the span outputs are not trivially 0 / 1


# ------------------------------------------------------------------------------------------------ 3. alone = in a batch; two calls
@pytest.mark.parametrize("name", ["one_wave_dpp", "one_wave_lds", "4_waves_L100"])
def test_a_clip_alone_equals_the_clip_in_a_batch_and_two_calls_agree(name):
    from lyricalignment_amd import _lib
    clips, refs, ys = cases(name)
    keys = ("occupancy", "onset_prob", "offset_prob", "log_z", "status", "visits", "span_skip", "repeat_count", "path_prob", "gamma")
    with _lib.option("viterbi_dpp", 0 if name == "one_wave_lds" else 1):
        first, second = _run(clips), _run(clips)
        for k in keys:
            assert first[k].tobytes() == second[k].tobytes(), (name, k)
        Lmax = max(len(c["lab"]) for c in clips)
        for b in (0, 1, len(clips) - 2, len(clips) - 1):
            c = clips[b]
            pad = dict(lab=[1] * Lmax, em=np.zeros((8, Lmax + 1), np.float32), skip=None, rf=None, kind="pad", T=0)    # keeps the kernel form
            alone = _run([c, pad])
            va, vb = _clip_view(alone, 0, c), _clip_view(first, b, c)
            for k in va:
                assert np.asarray(va[k]).tobytes() == np.asarray(vb[k]).tobytes(), (name, b, k)


# ------------------------------------------------------------------------------------------------ 4. a prohibitive penalty
@pytest.mark.parametrize("name", ["one_wave_dpp", "8_waves_L200"])
def test_a_prohibitive_repeat_penalty_gives_the_repeat_free_numbers(name):
    """repeat_penalty = 1e4: exp(-1e4) is 0, every return weighs nothing; onset / offset are the repeat-free DP's."""
    clips, _, _ = cases(name)
    clips = clips[:4]
    got = _run(clips, rpen=1e4, dp_repeat="null")
    assert any(c["rf"] is not None for c in clips)
    for b, c in enumerate(clips):
        r = rr.viterbi(c["em"], c["lab"], c["skip"], PEN, None, 0.0, rows=True)
        assert r[3] == rr.LA_OK and got["onset"][b, : len(c["lab"])].tolist() == r[0]
        y = yardstick(c, r, rf=None)
        _assert_close(got, b, c, y, (name, b, "barred"))
        assert not y["repeat_count"].any() and float(got["repeat_count"][b].max()) <= tol(c["em"].shape[0], 0.0)


# ------------------------------------------------------------------------------------------------ 5. edge spans
EDGES = dict(trs.EDGES)
EDGES["two spans sharing an end"] = ([1, 2, 3, 4, 5], [-1, 4, 4, -1, -1], None, [0, 1, 2, 3, 2, 3, 1, 2, 3, 4])


@functools.lru_cache(maxsize=None)
def edge_cases():
    clips, refs, ys = [], [], []
    for i, (name, (lab, rf, skip, sung)) in enumerate(EDGES.items()):
        hard = trs._edge_clip(lab, rf, skip, sung, 50 + 3 * i, i)
        for c in (hard, soften(hard, -2.0)):
            r = trs.reference(c, pen=0.0, rpen=0.25)
            assert r[3] == rr.LA_OK, name
            clips.append(dict(c, name=name)); refs.append(r); ys.append(yardstick(c, r, pen=0.0, rpen=0.25))
    return clips, refs, ys


@pytest.mark.parametrize("dpp", [1, 0])
def test_edge_spans(dpp):
    """(0, L), a one-label span, a span ending at L, equal first and last labels (no K-1 arc), nested, overlapping, two spans sharing an
    end, spans with optional lines: each planted hard (every return certain) and soft (off level -2: fractional counts)."""
    from lyricalignment_amd import _lib
    clips, refs, ys = edge_cases()
    for c, r, y in zip(clips, refs, ys):
        if not c["kind"].startswith("soft"):
            returns = [a for a, e in rpr.repeat_spans_of(c["rf"], len(c["lab"]))]
            assert r.n_repeats > 0 and y["repeat_count"][returns].min() > 0.9 and y["repeat_count"].sum() > r.n_repeats - 0.1, c["name"]
    soft = [y["repeat_count"].max() for c, y in zip(clips, ys) if c["kind"].startswith("soft")]
    assert sum(abs(x - round(x)) > 0.05 for x in soft) >= len(soft) // 2 and max(soft) > 2.0  # the soft twins are fractional; counts above 2
    with _lib.option("viterbi_dpp", dpp):
        got = _run(clips, pen=0.0, rpen=0.25)
    worst = {}
    for b, (c, y) in enumerate(zip(clips, ys)):
        _assert_close(got, b, c, y, (c["name"], c["kind"], dpp), worst)
        _assert_identity(got, b, c, (c["name"], c["kind"], dpp))
    print(f"dpp={dpp}: soft repeat_count maxima {[round(float(x), 3) for x in soft]}")
    print(f"dpp={dpp}: largest error / bound: " + ", ".join(f"{k} {f:.3f}" for k, (f, e) in worst.items()))


# ------------------------------------------------------------------------------------------------ 6. windows that allow only the second pass
@pytest.mark.parametrize("dpp", [1, 0])
def test_windows_that_allow_a_label_only_on_the_second_pass(dpp):
    """Label 1 is optional and lies inside the repeat span (0, 3); the audio sings 0 2 0 1 2 3.  The window of label 1's state opens at its
    visit on the second pass: on the first pass it can only be jumped.  Hard and soft (off level -1), the soft one also with the window
    narrowed at its end."""
    from lyricalignment_amd import _lib
    lab, rf, skip, sung = trs.EDGES["visit beats skip"]
    hard = trs._edge_clip(lab, rf, skip, sung, 60, 8)
    clips, wins, refs, ys = [], [], [], []
    for c, narrow in ((hard, False), (soften(hard, -1.0), False), (soften(hard, -1.0), True)):
        free = trs.reference(c, pen=0.0, rpen=0.25)
        T, S = c["em"].shape[0], 2 * len(lab) + 1
        lo, hi = [0] * S, [T] * S
        base = trs.reference(hard, pen=0.0, rpen=0.25)
        lo[3] = base[0][1]                          # label 1's onset on the hard clip: on its second pass
        if narrow:
            hi[3] = base[1][1] + 2
        r = trs.reference(c, lo, hi, pen=0.0, rpen=0.25)
        assert r[3] == rr.LA_OK and free[3] == rr.LA_OK
        clips.append(c); wins.append((lo, hi)); refs.append(r); ys.append(yardstick(c, r, pen=0.0, rpen=0.25, lo=lo, hi=hi))
    assert refs[0].n_repeats == 1 and refs[0].n_jumps == 1
    assert ys[0]["visits"][1] > 0.9 and ys[0]["repeat_count"][0] > 0.9 and ys[0]["span_skip"][2] > 0.9
    open_soft = yardstick(clips[1], refs[1], pen=0.0, rpen=0.25)
    # the window binds on the soft clip: without it the state holds more than one expected frame before the window opens
    assert open_soft["gamma"][: wins[1][0][3], 3].sum() > 1.0 and np.abs(open_soft["gamma"] - ys[1]["gamma"]).max() > 0.05
    assert not ys[1]["gamma"][: wins[1][0][3], 3].any() and 0.05 < ys[1]["repeat_count"][0]
    with _lib.option("viterbi_dpp", dpp):
        got = _run(clips, pen=0.0, rpen=0.25, windows=wins)
    for b, (c, y) in enumerate(zip(clips, ys)):
        _assert_close(got, b, c, y, ("second pass", b, dpp))
        _assert_identity(got, b, c, ("second pass", b, dpp))
        assert not got["gamma"][b, : wins[b][0][3], 3].any()


# ------------------------------------------------------------------------------------------------ 7. statuses and zeroed rows
@pytest.mark.parametrize("Lmax", [26, 100])
def test_statuses_and_zeroed_rows(Lmax):
    ok = make_clip(1, 60 if Lmax == 26 else 160, Lmax, "repeat")
    short = dict(make_clip(2, 60, 20, "repeat"), T=7)                   # 20 labels in 7 frames: too short
    empty = dict(lab=[], em=np.zeros((5, 1), dtype=np.float32), skip=None, rf=None, kind="empty")
    no_frames = dict(make_clip(3, 30, 8, "declared"), T=0)
    closed = make_clip(4, 50, 9, "repeat")
    clips = [ok, short, empty, no_frames, closed]
    wins = [rr._open(None, None, 2 * len(c["lab"]) + 1, c["em"].shape[0]) for c in clips]
    wins[4] = ([1] * 19, wins[4][1])                                     # row 0 closed: no path inside the windows
    got = _run(clips, windows=wins)
    r_ok = trs.reference(ok)
    _assert_close(got, 0, ok, yardstick(ok, r_ok), "ok")
    assert got["status"].tolist() == [rr.LA_OK, rr.LA_EINFEASIBLE, rr.LA_EEMPTY, rr.LA_EINVAL, rr.LA_EINFEASIBLE]
    assert np.isneginf(got["log_z"][1]) and np.isneginf(got["log_z"][4]) and got["log_z"][2] == 0.0 and got["log_z"][3] == 0.0
    for b in (1, 2, 3, 4):
        for k in ("occupancy", "onset_prob", "offset_prob", "visits", "span_skip", "repeat_count", "path_prob", "gamma"):
            assert not got[k][b].any(), (b, k)


# ------------------------------------------------------------------------------------------------ 8. the wrapper
def test_wrapper_refusals_and_optional_arguments():
    from lyricalignment_amd import ops
    em = torch.zeros((2, 30, 9), dtype=torch.float32).cuda()
    lab = (torch.arange(16, dtype=torch.int32).reshape(2, 8) + 1).cuda()
    n, t = torch.full((2,), 8, dtype=torch.int32).cuda(), torch.full((2,), 30, dtype=torch.int32).cuda()
    rf = torch.full((2, 8), -1, dtype=torch.int32).cuda()
    on, off, _, _, path = ops.viterbi_repeats_batch(em, lab, n, t, repeat_from=rf)
    for bad in (rf[:1], rf[:, :7], rf.long(), rf.cpu()):
        with pytest.raises(ValueError):
            ops.alignment_posteriors_repeats(em, lab, n, t, on, off, repeat_from=bad)
    for bad in (path[:1], path[:, :29], path.long(), path.cpu()):
        with pytest.raises(ValueError):
            ops.alignment_posteriors_repeats(em, lab, n, t, on, off, path=bad)
    for pen in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            ops.alignment_posteriors_repeats(em, lab, n, t, on, off, repeat_from=rf, repeat_penalty=pen)
    with pytest.raises(ValueError):
        ops.alignment_posteriors_repeats(em, lab, n, t, on, off, win_lo=torch.zeros((2, 17), dtype=torch.int32).cuda())
    with pytest.raises(ValueError):
        ops.alignment_posteriors_repeats(em, lab, n, t, on, off, boundary_window=-1)
    wide = (torch.zeros((1, 4, 513), dtype=torch.float32).cuda(), torch.ones((1, 512), dtype=torch.int32).cuda(), n[:1], t[:1])
    frames = torch.zeros((1, 512), dtype=torch.int32).cuda()
    with pytest.raises(NotImplementedError):
        ops.alignment_posteriors_repeats(*wide, frames, frames)
    res = ops.alignment_posteriors_repeats(em, lab, n, t, on, off)          # nothing optional given: no path, no path_prob
    assert len(res) == 9 and res[8] is None and not res[7].any() and (res[4] == 0).all()
    res = ops.alignment_posteriors_repeats(em, lab, n, t, on, off, path=path, want_gamma=True)
    assert len(res) == 10 and res[8].shape == (2, 30) and res[9].shape == (2, 30, 17)
    g = res[9].gather(2, path.long()[:, :, None])[:, :, 0]
    assert torch.equal(g, res[8])                                            # path_prob is gamma at the path, the same bits


# ------------------------------------------------------------------------------------------------ 9. the Python surface
tiny = trs.tiny            # the tiny random-weight model and clips of tests/test_gpu_repeat_spans.py
REPEATS, OPTIONAL = trs.REPEATS, trs.OPTIONAL
SHARED = ("occupancy", "onset_prob", "offset_prob", "path_log_posterior", "span_skip_prob")


def _scores_close(got, want, T, what):
    """Two routes to one clip's dict: the fused head's emissions and la_emissions_from_logits' differ in their last bits, so the numbers agree
    within the kernel test's bound (window_log_prob, a difference of two log_z, within twice that), as the older confidence tests have it."""
    assert set(got) == set(want), what
    worst = 0.0
    for k, w in want.items():
        g = got[k]
        if k == "repeat_count":
            assert list(g) == list(w), what
            g, w = list(g.values()), list(w.values())
        g, w = np.atleast_1d(np.asarray(g, np.float64)), np.atleast_1d(np.asarray(w, np.float64))
        assert g.shape == w.shape, (what, k)
        if g.size:
            frac = float(np.max(np.abs(g - w) / (tol(T, np.abs(w)) * (2 if k == "window_log_prob" else 1))))
            worst = max(worst, frac)
            assert frac <= 1.0, (what, k, g, w)
    return worst


def _check_scores(seconds, segments, scores, repeats, optional, windows):
    for b, (res, seg, d) in enumerate(zip(seconds, segments, scores)):
        L = len(res)
        assert set(d) == set(SHARED) | {"visits", "repeat_count", "visit_occupancy"} | ({"window_log_prob"} if windows else set()), (b, sorted(d))
        assert len(d["visits"]) == L and len(d["occupancy"]) == L and len(d["onset_prob"]) == L and len(d["offset_prob"]) == L
        assert list(d["repeat_count"]) == [tuple(s) for s in repeats[b]] and all(v >= 0.0 for v in d["repeat_count"].values())
        assert len(d["span_skip_prob"]) == len(optional[b] if optional else [])
        assert len(d["visit_occupancy"]) == len(seg) and all(0.0 <= v <= 1.0 + 1e-6 for v in d["visit_occupancy"])
        assert d["path_log_posterior"] <= 1e-6
        # the first visit's occupancy is the reported occupancy: the mean of gamma at the path over the same frames
        firsts = {}
        for i, (n, _, _) in enumerate(seg):
            firsts.setdefault(n, i)
        for n, i in firsts.items():
            assert abs(d["visit_occupancy"][i] - d["occupancy"][n]) < 1e-5, (b, n)
        # the identity, label by label: every term within the kernel test's bound at T <= 2000 frames (the longest clip here has 1650)
        left, right = rpr.identity_sides(d["visits"], [0.0] * (L + 1), [0.0] * L, None, None)
        bound = tol(2000, left)
        for (a, n), v in zip(optional[b] if optional else [], d["span_skip_prob"]):
            left[a:n] += v
            bound[a:n] += tol(2000, v)
        for (a, e), v in d["repeat_count"].items():
            right[a:e] += v
            bound[a:e] += tol(2000, v)
        assert (np.abs(left - right) <= bound).all(), (b, left, right)


@pytest.mark.parametrize("use_ctc", [True, False])
def test_align_with_repeat_confidence_equals_the_two_step_route(tiny, use_ctc):
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels = tiny["model"], tiny["audios"], tiny["labels"]
    two = ua.perform_viterbi_ctc_repeat_scored if use_ctc else ua.perform_viterbi_repeat_scored
    anchors = [[(4, 1.0, 0.5)], [], [], []]
    with torch.no_grad():
        logits, _ = model.frame_manual_forward(audios)
        for kw in (dict(repeat_spans=REPEATS), dict(repeat_spans=REPEATS, repeat_penalty=2.0),
                   dict(repeat_spans=REPEATS, optional_spans=OPTIONAL, skip_penalty=0.5),
                   dict(repeat_spans=REPEATS, onset_anchors=anchors),
                   dict(repeat_spans=REPEATS, optional_spans=OPTIONAL, skip_penalty=0.5, onset_anchors=anchors)):
            fused = model.align(audios, labels, use_ctc=use_ctc, return_segments=True, return_repeat_confidence=True, **kw)
            steps = two(logits, labels, return_segments=True, **kw)
            assert len(fused) == 3 and len(steps) == 3 and fused[:2] == steps[:2]                            # seconds and segments: exactly
            worst = max(_scores_close(g, w, logits.shape[1], (use_ctc, sorted(kw), b)) for b, (g, w) in enumerate(zip(fused[2], steps[2])))
            print(f"use_ctc={use_ctc} {sorted(kw)}: fused against two steps, largest difference {worst:.3f} of the bound")
            short = model.align(audios, labels, use_ctc=use_ctc, return_repeat_confidence=True, **kw)
            assert len(short) == 2 and short[0] == fused[0] and short[1] == fused[2]
            short2 = two(logits, labels, **kw)
            assert len(short2) == 2 and short2[0] == steps[0] and short2[1] == steps[2]
            assert fused[:2] == model.align(audios, labels, use_ctc=use_ctc, return_segments=True, **kw)      # the DP's result is untouched
            _check_scores(*fused, REPEATS, kw.get("optional_spans"), "onset_anchors" in kw)
            frames = model.align(audios, labels, use_ctc=use_ctc, return_frames=True, return_repeat_confidence=True, **kw)
            assert len(frames) == (12 if "onset_anchors" in kw else 11) and frames[-1].dtype == torch.int32
        print(f"use_ctc={use_ctc}: visits {[[round(v, 2) for v in d['visits']] for d in fused[2]]}")
        print(f"use_ctc={use_ctc}: repeat_count {[d['repeat_count'] for d in fused[2]]}")


def test_per_clip_and_long_form_with_repeat_confidence(tiny):
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels, tr = tiny["model"], tiny["audios"], tiny["labels"], tiny["tr"]
    with torch.no_grad():
        batch = model.align(audios, labels, per_clip=True, repeat_spans=REPEATS, optional_spans=OPTIONAL, return_segments=True,
                            return_repeat_confidence=True)
        for r, i in enumerate(tiny["idx"]):
            alone = model.align([audios[r]], tr._clip_labels(i), per_clip=True, repeat_spans=[REPEATS[r]], optional_spans=[OPTIONAL[r]],
                                return_segments=True, return_repeat_confidence=True)
            assert batch[0][r] == alone[0][0] and batch[1][r] == alone[1][0], i
            _scores_close(batch[2][r], alone[2][0], 1500, ("per_clip", i))
        audio = np.concatenate([tr._clip(4), tr._clip(3)])                                     # 33 s: two encoder chunks
        lab = torch.from_numpy(np.random.RandomState(5).randint(2, 403, size=(1, 14)))
        kw = dict(repeat_spans=[[(3, 7)]], optional_spans=[[(10, 14)]], return_segments=True)
        logits, _ = model.frame_manual_forward([audio])
        assert logits.shape[1] > 1500
        got = model.align([audio], lab, return_repeat_confidence=True, **kw)
        steps = ua.perform_viterbi_ctc_repeat_scored(logits, lab, **kw)
        assert got[:2] == steps[:2]
        _scores_close(got[2][0], steps[2][0], logits.shape[1], "long form")
        _check_scores(*got, [[(3, 7)]], [[(10, 14)]], False)


def test_without_a_repeat_span_the_shared_numbers_are_the_sheet_confidence(tiny):
    model, audios, labels = tiny["model"], tiny["audios"], tiny["labels"]
    anchors = [[(4, 1.0, 0.5)], [], [], []]
    with torch.no_grad():
        for kw in (dict(), dict(optional_spans=OPTIONAL, skip_penalty=0.5), dict(optional_spans=OPTIONAL, skip_penalty=0.5, onset_anchors=anchors)):
            want_s, want = model.align(audios, labels, return_sheet_confidence=True, **kw)
            for rep in (None, [[], [], [], []]):
                got_s, got = model.align(audios, labels, return_repeat_confidence=True, repeat_spans=rep, **kw)
                assert got_s == want_s
                for b, (g, w) in enumerate(zip(got, want)):
                    for k in SHARED:
                        assert g[k] == w[k], (b, k)
                    assert g["visits"] == w["sung_prob"] and g["repeat_count"] == {}
                    if "onset_anchors" in kw:
                        assert g["window_log_prob"] == w["window_log_prob"]


def test_align_record_lines_with_visit_confidence_and_the_old_refusals(tiny):
    from lyricalignment_amd.harness import PinyinClassLUT, align_record_lines
    from lyricalignment_amd.utils import alignment as ua
    from test_gpu_parity_full import VOCAB
    model, tr, audios, labels = tiny["model"], tiny["tr"], tiny["audios"], tiny["labels"]
    lut = PinyinClassLUT([str(i) for i in range(VOCAB)], {str(i): i for i in range(VOCAB)})           # token id -> the same class id
    ids_all = [int(v) for v in tr._clip_labels(0)[0]]                                                 # 11 labels: lines of 3 / 4 / 2 / 2
    lines = ["".join(chr(0x4E00 + 11 * k + j) for j in range(n)) for k, n in enumerate((3, 4, 2, 2))]
    ids, pos = {}, 0
    for line in lines:
        ids[line] = ids_all[pos: pos + len(line)]
        pos += len(line)
    optional, repeatable = [False, False, True, False], [False, True, False, True]
    args = (model, tr._clip(0), lines, optional, lut, lambda t: ids[t])
    occ, conf = align_record_lines(*args, repeatable=repeatable, repeat_penalty=0.0, with_visit_confidence=True)
    assert occ == align_record_lines(*args, repeatable=repeatable, repeat_penalty=0.0)
    assert len(conf) == 4
    for i, c in enumerate(conf):
        assert set(c) == {"visits", "repeat_count", "occurrence_occupancy"} and c["visits"] >= 0.0
        assert (c["repeat_count"] is not None and c["repeat_count"] >= 0.0) if repeatable[i] else c["repeat_count"] is None
        assert len(c["occurrence_occupancy"]) == len(occ[i]) and all(0.0 <= v <= 1.0 + 1e-6 for v in c["occurrence_occupancy"])
    print(f"lines sung {[round(c['visits'], 3) for c in conf]}, returns {[c['repeat_count'] for c in conf]}")
    # the old refusals still hold
    with pytest.raises(ValueError):
        align_record_lines(*args, repeatable=repeatable, with_confidence=True)
    with pytest.raises(ValueError):
        align_record_lines(*args, with_visit_confidence=True)
    with torch.no_grad():
        for kw in (dict(return_confidence=True), dict(return_span_confidence=True), dict(return_anchored_confidence=True),
                   dict(return_sheet_confidence=True)):
            with pytest.raises(ValueError):
                model.align(audios, labels, repeat_spans=REPEATS, **kw)
            with pytest.raises(ValueError):
                model.align(audios, labels, return_repeat_confidence=True, **kw)
        logits, _ = model.frame_manual_forward(audios)
    for scored in (ua.perform_viterbi_ctc_scored, ua.perform_viterbi_scored, ua.perform_viterbi_ctc_anchored_scored, ua.perform_viterbi_ctc_sheet_scored):
        with pytest.raises(ValueError):
            scored(logits, labels, repeat_spans=REPEATS)
    with pytest.raises(ValueError):
        ua.anchored_alignment_loss(logits, labels, repeat_spans=REPEATS)
    rows = torch.zeros((4, 11), dtype=torch.int32)
    for kind in ("plain", "span", "anchored", "sheet"):
        with pytest.raises(ValueError):
            ua.run_lattice(*[None] * 4, confidence=kind, repeat_from=rows)
    with pytest.raises(NotImplementedError):
        ua.perform_viterbi_ctc_repeat_scored(torch.zeros((1, 8, 12)).cuda(), torch.ones((1, 512), dtype=torch.int64), repeat_spans=[[(0, 2)]])
    with pytest.raises(NotImplementedError):
        model.align(audios[:1], torch.ones((1, 512), dtype=torch.int64), return_repeat_confidence=True)
