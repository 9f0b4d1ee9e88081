"""tools/benchlib.py without a GPU: the planted emissions and the window helpers against a restatement, the verdict against the parent at
and one ulp beyond its bounds, the C argument list of every lattice leg against _lib.SYMBOLS and against the call ops makes for the same
inputs (a recorder stands for the library, CPU tensors for device tensors, as in tests/test_host_ops_lattice_args.py), and that importing
a bench tool does nothing."""
import importlib
import itertools
import math
import os
import sys

import pytest
import torch

from test_host_ops_lattice_args import STREAM, _parameters, _StandIn

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
import benchlib as bl  # noqa: E402

B, T, L = 2, 6, 2
DP = ("viterbi", "viterbi_spans", "viterbi_windows", "viterbi_lattice", "viterbi_repeats", "viterbi_lines", "viterbi_min_duration")
POST = ("alignment_posteriors", "alignment_posteriors_spans", "alignment_posteriors_windows", "alignment_posteriors_lattice",
        "alignment_posteriors_repeats", "alignment_posteriors_song", "alignment_posteriors_lines")
# what a tile entry takes: the keyword of its row tensor and of its scalar in ops' public function, the scalar the legs are given
TILE = {"viterbi_lines": ("line_start", "line_jump_penalty", 1.5), "viterbi_min_duration": ("min_frames", "max_min_frames", 3),
        "alignment_posteriors_lines": ("line_start", "line_jump_penalty", 1.5)}
KERNEL_TOOLS = ("optional_spans_bench", "anchored_bench", "wide_lattice_bench", "repeat_lattice_bench", "dp_ab_bench", "span_confidence_bench",
                "anchored_confidence_bench", "wide_confidence_bench", "repeat_confidence_bench", "song_confidence_bench")
MODEL_TOOLS = ("confidence_bench", "readings_bench", "pronunciation_bench", "anchored_loss_bench")
# the C parameters a leg fills with addresses of its own (include/lyricalign.h's names): a sweep's onset / offset are inputs
OWN = {"final_score", "status", "occupancy", "onset_prob", "offset_prob", "present_prob", "visits", "in_order", "span_skip_prob", "repeat_count",
       "path_prob", "log_z", "workspace"}


@pytest.mark.parametrize("B_, T_, L_, sung", [(2, 40, 3, [0, 1, 2]), (1, 90, 5, [0, 1, 2, 1, 2, 3, 4])])
def test_planted_is_the_recipe(B_, T_, L_, sung):
    seed = B_ + T_ + L_
    g = torch.Generator().manual_seed(seed)
    want = -torch.rand((B_, T_, L_ + 1), generator=g) * 12 - 1
    seg = T_ // (2 * len(sung) + 1)
    assert seg >= 4
    for i, n in enumerate(sung):
        want[:, (2 * i + 1) * seg:(2 * i + 2) * seg, 1 + n] += 9.6
    for i in range(len(sung) + 1):
        want[:, 2 * i * seg:(2 * i + 1) * seg, 0] += 9.6
    got = bl.planted(B_, T_, L_, sung, seed, "cpu")
    assert got.dtype == torch.float32 and got.numpy().tobytes() == want.numpy().tobytes()
    labels, n_labels, n_frames = bl.sheet(B_, T_, L_, "cpu")
    assert labels.tolist() == [list(range(1, L_ + 1))] * B_ and n_labels.tolist() == [L_] * B_ and n_frames.tolist() == [T_] * B_
    assert labels.dtype == n_labels.dtype == n_frames.dtype == torch.int32


def test_lines_and_windows():
    from lyricalignment_amd.utils.alignment import windows_from_anchors
    L_, T_ = 5, 120
    assert bl.lines_of(L_, 2) == ([2, 2, 1], [0, 2, 4]) and bl.lines_of(4, 2) == ([2, 2], [0, 2])
    assert bl.sung_lines([2, 2, 1], [1, 2, 0]) == [0, 1, 2, 3, 2, 3]
    lo, hi = bl.open_windows(2, T_, L_, "cpu")
    assert lo.dtype == hi.dtype == torch.int32 and lo.tolist() == [[0] * 11] * 2 and hi.tolist() == [[T_] * 11] * 2
    onsets = torch.tensor([[10, 20, 40, 50, 90], [30, 35, -1, -1, -1]], dtype=torch.int32)      # clip 1: lines 2 and 3 left out, none after
    want = [windows_from_anchors(L_, T_, onset_anchors=[(4, 90 * 0.02, 0.5), (2, 40 * 0.02, 0.5), (0, 10 * 0.02, 0.5)]),
            windows_from_anchors(L_, T_, onset_anchors=[(4, (T_ - 1) * 0.02, 0.5), (2, (T_ - 1) * 0.02, 0.5), (0, 30 * 0.02, 0.5)])]
    lo, hi = bl.anchored_windows(onsets, [0, 2, 4], T_, L_, 0.5)
    assert lo.dtype == hi.dtype == torch.int32
    assert lo.tolist() == [list(w[0]) for w in want] and hi.tolist() == [list(w[1]) for w in want]
    assert lo[0].tolist() != [0] * 11                                                              # the anchors do narrow something


def test_against_parent_bounds():
    lo, hi = 1.25, 1.5
    for m in (lo, hi, 1.3):
        line = bl.against_parent("leg", (m, 0.0, 9.0), (1.4, lo, hi))
        assert bl.inside((m, 0.0, 9.0), (1.4, lo, hi))
        assert line == f"leg: {m:.3f} against the parent's 1.400 (1.250 .. 1.500): inside its min .. max ({100 * (m / 1.4 - 1):+.1f} % of its median)"
    below, above = math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf)
    assert not bl.inside((below, 0, 9), (1.4, lo, hi)) and not bl.inside((above, 0, 9), (1.4, lo, hi))
    assert f": BELOW by {lo - below:.3f} ms its min .. max (-10.7 % of its median)" in bl.against_parent("leg", (below, 0, 9), (1.4, lo, hi))
    assert f": ABOVE by {above - hi:.3f} ms its min .. max (+7.1 % of its median)" in bl.against_parent("leg", (above, 0, 9), (1.4, lo, hi))
    assert ": BELOW by 0.250 ms its" in bl.against_parent("leg", (1.0, 0, 9), (1.4, lo, hi))
    assert ": ABOVE by 0.500 ms its" in bl.against_parent("leg", (2.0, 0, 9), (1.4, lo, hi))
    lines = bl.against_parent_processes("k", [[1.0, 1.0], [1.2, 1.2]], [[1.0, 1.0], [1.1, 1.1]])
    assert len(lines) == 3 and "spread between the parent's processes 0.100" in lines[1] and "inside the parent's spread: equal" in lines[2]
    assert "SLOWER: a regression" in bl.against_parent_processes("k", [[2.0], [2.0]], [[1.0], [1.1]])[2]
    assert "FASTER" in bl.against_parent_processes("k", [[0.5], [0.5]], [[1.0], [1.1]])[2]


def test_stat_and_report(tmp_path, capsys):
    assert bl.stat([3.0, 1.0, 2.0]) == (2.0, 1.0, 3.0)
    assert bl.timed("leg", (2.0, 1.0, 3.0), 5) == "leg      2.000 (1.000 .. 3.000)"
    report = bl.Report(str(tmp_path / "sub" / "out.txt"))
    report.say("a")
    report.say()
    report.close()
    assert capsys.readouterr().out == "a\n\n" and (tmp_path / "sub" / "out.txt").read_text() == "a\n\n"
    args = bl.parse(bl.parser(parent_lib=True, quick=True), ["--quick"])
    assert args.runs == 2 and args.parent_lib == "" and bl.parse(bl.parser(quick=True), []).runs == 30
    assert bl.parse(bl.parser(quick=True), ["--quick", "--runs", "7"]).runs == 7


def _inputs():
    """Every tensor with a row pitch of its own, so that a stride in the wrong place shows."""
    i32 = dict(dtype=torch.int32)
    d = dict(em=torch.zeros((B, T + 1, L + 3))[:, :T, : L + 1], labels=torch.ones((B, L + 4), **i32)[:, :L],
             n_labels=torch.full((B,), L, **i32), n_frames=torch.full((B,), T, **i32),
             onset=torch.zeros((B, L), **i32), offset=torch.ones((B, L), **i32),
             skip=torch.full((B, L + 6), -1, **i32)[:, : L + 1], win_lo=torch.zeros((B, 2 * L + 8), **i32)[:, : 2 * L + 1],
             win_hi=torch.full((B, 2 * L + 8), T, **i32)[:, : 2 * L + 1], repeat=torch.full((B, L + 3), -1, **i32)[:, :L],
             path=torch.zeros((B, T + 5), **i32)[:, :T], row=torch.ones((B, L + 7), **i32)[:, :L])
    assert len({d[k].stride(0) for k in ("em", "labels", "skip", "win_lo", "repeat", "path", "row")}) == 7
    return d


def _admitted(stem):
    """(skip, windows, repeat, path given or not) in every combination the entry admits: an entry named for its argument always gets it."""
    from lyricalignment_amd import ops
    e = ops._entry(stem)
    skip = (True,) if stem.endswith("_spans") else (False, True) if e.spans else (False,)
    windows = (True,) if stem.endswith("_windows") else (False, True) if e.windows else (False,)
    repeat = (False, True) if e.repeats else (False,)
    path = (False, True) if (e.repeats or e.row) and stem in POST else (False,)
    return list(itertools.product(skip, windows, repeat, path))


def test_every_combination_is_covered():
    assert sum(len(_admitted(s)) for s in DP) == 1 + 1 + 2 + 4 + 8 + 1 + 1 and sum(len(_admitted(s)) for s in POST) == 1 + 1 + 2 + 4 + 16 + 16 + 2
    from lyricalignment_amd import ops
    assert set(DP + POST) == set(ops._ENTRIES) | set(ops._TILE_ENTRIES) and len(DP + POST) == 14 and set(TILE) == set(ops._TILE_ENTRIES)


@pytest.fixture
def stand_ins(monkeypatch):
    from lyricalignment_amd import _lib, ops
    theirs = _StandIn()
    monkeypatch.setattr(ops, "lib", lambda: theirs)
    monkeypatch.setattr(ops, "_dev", lambda t, name, dtype=None: None)
    monkeypatch.setattr(ops, "stream_ptr", lambda: STREAM)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: STREAM)
    return _StandIn(), theirs


@pytest.mark.parametrize("stem", DP + POST)
def test_the_c_call_of_every_leg(stand_ins, stem):
    from lyricalignment_amd import _lib, ops
    ours, theirs = stand_ins
    d = _inputs()
    c = bl.case(d["em"], d["labels"], d["n_labels"], d["n_frames"])
    assert (c.B, c.T, c.L) == (B, T, L)
    symbol = "la_" + stem + ("_batch" if stem in DP else "")
    names, _ = _parameters(symbol)
    argtypes = _lib.SYMBOLS[symbol][1]
    row_kw, scalar_kw, scalar = TILE.get(stem, (None, None, None))
    tile = dict(row=d["row"], scalar=scalar) if stem in TILE else {}
    dims = (B, T, L) + ((scalar,) if stem == "viterbi_min_duration" else ())
    assert len(_lib.SYMBOLS[f"la_{stem}_workspace_bytes"][1]) == len(dims) + 1                        # the query's own dimensions, then &need
    for skip_given, win_given, repeat_given, path_given in _admitted(stem):
        skip = d["skip"] if skip_given else None
        windows = (d["win_lo"], d["win_hi"]) if win_given else None
        repeat = d["repeat"] if repeat_given else None
        path = d["path"] if path_given else None
        del ours.calls[:], ours.queries[:], theirs.calls[:], theirs.queries[:]
        if stem in DP:
            fn, out = bl.dp_leg(ours, stem, c, skip, windows, repeat, **tile)
        else:
            fn, out = bl.posterior_leg(ours, stem, c, (d["onset"], d["offset"]), skip, windows, repeat, path, boundary_window=2, **tile)
        assert ours.calls == [] and ours.queries == [(f"la_{stem}_workspace_bytes", dims)]            # the leg's own query, nothing launched yet
        assert all(float(t.double().min()) == float(t.double().max()) == -7 for t in out.values())
        fn()
        fn()
        assert [name for name, _ in ours.calls] == [symbol] * 2 and ours.calls[0][1] == ours.calls[1][1]
        got = ours.calls[0][1]
        assert len(got) == len(argtypes) == len(names)
        for a, argtype in zip(got, argtypes):
            argtype.from_param(a)                                                                      # raises on an argument ctypes would refuse
        takes = ops._entry(stem)
        kw = {row_kw: d["row"], scalar_kw: scalar} if stem in TILE else {}
        if takes.spans:
            kw.update(skip_from=skip, skip_penalty=0.0)
        if windows is not None:
            kw.update(win_lo=windows[0], win_hi=windows[1])
        if takes.repeats:
            kw.update(repeat_from=repeat, repeat_penalty=0.0)
        if stem in POST:
            kw.update(boundary_window=2, want_gamma=False, **(dict(path=path) if takes.repeats or takes.row else {}))
        frames = (d["onset"], d["offset"]) if stem in POST else ()
        getattr(ops, stem + "_batch" if stem in DP else stem)(d["em"], d["labels"], d["n_labels"], d["n_frames"], *frames, **kw)
        assert [name for name, _ in theirs.calls] == [symbol] and theirs.queries == [(f"la_{stem}_workspace_bytes", dims)]
        want = theirs.calls[0][1]
        own = OWN | ({"onset", "offset", "path"} if stem in DP else set())
        mine = dict(onset=out.get("onset"), offset=out.get("offset"), final_score=out.get("score"), status=out["status"], path=out.get("path"),
                    occupancy=out.get("occupancy"), onset_prob=out.get("onset_prob"), offset_prob=out.get("offset_prob"),
                    present_prob=out.get("present"), visits=out.get("visits", out.get("present")), in_order=out.get("in_order"),
                    span_skip_prob=out.get("span_skip"),
                    repeat_count=out.get("repeat_count"), path_prob=out.get("path_prob"), log_z=out.get("log_z"))
        for name, a, w in zip(names, got, want):
            where = (stem, skip_given, win_given, repeat_given, path_given, name)
            if name not in own:
                assert type(a) is type(w) and a == w, where
            elif name == "workspace":
                assert a != 0 and w != 0, where
            else:                                         # the leg's own tensor where ops passes its own, null where ops passes null
                assert (a == 0) == (w == 0) and a == (0 if mine[name] is None else mine[name].data_ptr()), where
        if "span_skip" in out:                            # the pitch the kernel is told for skip_from holds for span_skip_prob
            assert out["span_skip"].stride(0) == got[names.index("skip_stride")] and out["span_skip"].shape == (B, L + 1)
        if "path_prob" in out:
            assert out["path_prob"].stride(0) == got[names.index("path_stride")] and out["path_prob"].shape == (B, T)
        assert ("path_prob" in out) == (path is not None and bool(takes.repeats or takes.row))


def test_same_bits_and_a_failing_call():
    a = dict(x=torch.tensor([0.0, float("nan")]), status=torch.zeros(2, dtype=torch.int32))
    b = dict(x=torch.tensor([0.0, float("nan")]), status=torch.zeros(2, dtype=torch.int32))
    assert bl.same_bits(a, b, ("x", "status")) and bl.ok(a)
    b["x"][0] = -0.0
    b["status"][1] = 2
    assert not bl.same_bits(a, b, ("x",)) and not bl.ok(b)

    class Failing(_StandIn):
        def __getattr__(self, name):
            if name == "la_last_error":
                return lambda: b"the entry's own words"
            if name == "la_viterbi_batch":
                return lambda *args: 1
            return super().__getattr__(name)

    d = _inputs()
    fn, _ = bl.dp_leg(Failing(), "viterbi", bl.case(d["em"], d["labels"], d["n_labels"], d["n_frames"]))
    import lyricalignment_amd._lib as _lib
    stream, _lib.stream_ptr = _lib.stream_ptr, lambda: STREAM
    try:
        with pytest.raises(AssertionError, match="the entry's own words"):
            fn()
    finally:
        _lib.stream_ptr = stream


@pytest.mark.parametrize("tool", KERNEL_TOOLS + MODEL_TOOLS)
def test_importing_a_tool_does_nothing(tool, monkeypatch):
    """Also all the suite does for the four tools that run a model as well (MODEL_TOOLS): tests/test_gpu_bench_tools.py runs the ten others."""
    from lyricalignment_amd import _lib
    monkeypatch.setattr(sys, "argv", ["prog", "--no-such-flag"])          # a module that parsed it at import would exit
    monkeypatch.setattr(_lib, "_lib", None)
    sys.modules.pop(tool, None)
    module = importlib.import_module(tool)
    assert _lib._lib is None and not torch.cuda.is_initialized()
    assert callable(module.main) and module.main.__code__.co_varnames[0] == "argv" and module.main.__defaults__ == (None,)
    if tool in KERNEL_TOOLS:
        for quick in (False, True):
            table = module.leg_table(quick)
            assert table and all(len(set(names)) == len(names) >= 2 for names in table)
