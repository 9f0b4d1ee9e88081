"""utils.alignment.run_lattice without a GPU, on all seven kinds of confidence: with the eleven ops.* lattice calls replaced by recorders,
the calls it makes for every (confidence, spans, windows, repeat_from, more than 511 labels) are the route this file restates as data
(WANTED and the two rules under it; nothing here is read from the production table), in order, with the DP's frames and path, the
spans, the windows, the penalties and boundary_window handed on and the windows dropped in the free sweep; the result carries each
call's outputs in its fields; and the three refusals come before any call.  The production table agrees with
tests/test_gpu_lattice_dispatch.py's DISPATCH on DISPATCH's keys."""
import inspect

import pytest
import torch

from test_gpu_lattice_dispatch import DISPATCH, FIELDS

B, T = 2, 6
V, VS, VW, VL, VR = "viterbi_batch", "viterbi_spans_batch", "viterbi_windows_batch", "viterbi_lattice_batch", "viterbi_repeats_batch"
P, PS, PW, PL = "alignment_posteriors", "alignment_posteriors_spans", "alignment_posteriors_windows", "alignment_posteriors_lattice"
PR, PG = "alignment_posteriors_repeats", "alignment_posteriors_song"
DP, POST = (V, VS, VW, VL, VR), (P, PS, PW, PL, PR, PG)
OLDER_POST = (P, PS, PW)                   # boundary_window goes to these positionally, and no argument by keyword
KINDS = (None, "plain", "span", "anchored", "sheet", "repeat", "song")

# kind -> per (spans given, windows given): (DP entry, posteriors entry, log_z_free: None, "log_z" = the sweep's own, or the entry called
# once more without windows).  Up to 511 labels, no repeat_from.  ("span" with windows sweeps for a log_z_free its result does not hold.)
FACES = ((False, False), (True, False), (False, True), (True, True))
WANTED = {
    None: ((V, None, None), (VS, None, None), (VW, None, None), (VW, None, None)),
    "plain": ((V, P, None), (VS, P, None), (VW, P, None), (VW, P, None)),
    "span": ((V, PS, None), (VS, PS, None), (VW, PW, P), (VW, PW, PS)),
    "anchored": ((V, PS, "log_z"), (VS, PS, "log_z"), (VW, PW, P), (VW, PW, PS)),
    "sheet": ((V, PL, "log_z"), (VS, PL, "log_z"), (VW, PL, PL), (VW, PL, PL)),
    "repeat": ((VR, PR, None), (VR, PR, None), (VR, PR, PR), (VR, PR, PR)),
    "song": ((VR, PG, None), (VR, PG, None), (VR, PG, PG), (VR, PG, PG)),
}
NARROW = ("plain", "span", "anchored", "repeat")           # NotImplementedError beyond 511 labels
FILLED = {None: 4, "plain": 8, "span": 10, "anchored": 11, "sheet": 11, "repeat": 10, "song": 10}      # (+ log_z_free where a sweep is named)


def _wanted(kind, spans, windows, wide, repeats):
    """WANTED's row under the two rules: a given repeat_from sends the DP to viterbi_repeats_batch, and beyond 511 labels the DP's span
    and window entries give way to viterbi_lattice_batch."""
    dp, post, free = WANTED[kind][FACES.index((spans, windows))]
    if repeats:
        dp = VR
    if wide and dp in (VS, VW):
        dp = VL
    return dp, post, free


@pytest.fixture
def calls(monkeypatch):
    """Every ops lattice entry replaced by a recorder: log of (name, arguments by parameter name, the keywords used, the outputs)."""
    from lyricalignment_amd import ops
    log = []

    def recorder(name, signature):
        def call(*args, **kw):
            bound = signature.bind(*args, **kw)
            bound.apply_defaults()
            nb, L = args[1].shape
            if name in DP:
                out = (torch.zeros((nb, L), dtype=torch.int32), torch.ones((nb, L), dtype=torch.int32), torch.zeros((nb,), dtype=torch.float64),
                       torch.zeros((nb,), dtype=torch.int32))
                out += (torch.ones((nb, args[0].shape[1]), dtype=torch.int32),) if name == VR else ()
            else:
                out = tuple(torch.zeros((nb, L)) for _ in range(3)) + (torch.zeros((nb,), dtype=torch.float64), torch.zeros((nb,), dtype=torch.int32))
                out += (torch.zeros((nb, L)), torch.zeros((nb, L + 1))) if name != P else ()
                if name in (PR, PG):
                    out += (torch.zeros((nb, L)), None if bound.arguments["path"] is None else torch.zeros((nb, args[0].shape[1])))
            log.append((name, dict(bound.arguments), sorted(kw), out))
            return out
        return call
    for name in DP + POST:
        monkeypatch.setattr(ops, name, recorder(name, inspect.signature(getattr(ops, name))))
    return log


def _inputs(L):
    em, lab = torch.zeros((B, T, L + 1)), torch.ones((B, L), dtype=torch.int32)
    n_lab, nf = torch.full((B,), L, dtype=torch.int32), torch.full((B,), T, dtype=torch.int32)
    skip = torch.full((B, L + 1), -1, dtype=torch.int32)
    skip[0, 2] = 0
    win = (torch.zeros((B, 2 * L + 1), dtype=torch.int32), torch.full((B, 2 * L + 1), T, dtype=torch.int32))
    rep = torch.full((B, L), -1, dtype=torch.int32)
    rep[1, 0] = 2
    return em, lab, n_lab, nf, skip, win, rep


def test_the_production_table_says_what_the_dispatch_test_says():
    from lyricalignment_amd.utils import alignment as ua
    assert set(DISPATCH) <= set(ua.ROUTES) and len(DISPATCH) == 11
    for key, row in DISPATCH.items():
        assert tuple(ua.ROUTES[key]) == row, key
        assert _wanted(*key, False, False) == row, key                       # and so does this file's restatement
    assert set(ua.ROUTES) == {(kind, s, w) for kind in KINDS for s, w in FACES}
    for (kind, s, w), row in ua.ROUTES.items():
        for wide in (False, True):
            for repeats in (False, True):
                assert tuple(ua.route_of(kind, s, w, wide, repeats)) == _wanted(kind, s, w, wide, repeats), (kind, s, w, wide, repeats)


@pytest.mark.parametrize("head_dp", [False, True], ids=["", "dp_given"])
@pytest.mark.parametrize("L", [3, 600], ids=["", "wide"])
@pytest.mark.parametrize("has_rep", [False, True], ids=["", "repeat_from"])
@pytest.mark.parametrize("has_spans,has_win", FACES, ids=["no_face", "spans", "windows", "spans_windows"])
@pytest.mark.parametrize("kind", KINDS)
def test_run_lattice_takes_the_route_and_hands_everything_on(calls, kind, has_spans, has_win, has_rep, L, head_dp):
    from lyricalignment_amd.utils import alignment as ua
    em, lab, n_lab, nf, skip, win, rep = _inputs(L)
    given = tuple(torch.full(s, 9, dtype=torch.int32) for s in ((B, L), (B, L), (B,), (B,)))
    run = lambda: ua.run_lattice(em, lab, n_lab, nf, skip if has_spans else None, win if has_win else None, 1.5, kind, 3,
                                 dp=given if head_dp else None, repeat_from=rep if has_rep else None, repeat_penalty=0.25)
    # ---- the refusals, before any call (an older kind on the lattice with repeatable spans first, then the label limit)
    if has_rep and kind in ("plain", "span", "anchored", "sheet"):
        with pytest.raises(ValueError, match="repeat_from does not go with the four older kinds"):
            run()
        assert calls == []
        return
    if L > 511 and kind in NARROW:
        with pytest.raises(NotImplementedError, match=f"run_lattice: {L} labels exceed the 511-label limit of"):
            run()
        assert calls == []
        return
    r = run()
    dp_name, post_name, free_name = _wanted(kind, has_spans, has_win, L > 511, has_rep)
    takes_given = head_dp and dp_name == V                                  # a DP result that exists is the plain lattice's only
    sweeps = [n for n in (post_name, free_name) if n not in (None, "log_z")]
    assert [c[0] for c in calls] == ([] if takes_given else [dp_name]) + sweeps
    dp = given if takes_given else calls[0][3]
    assert len(dp) == (5 if dp_name == VR else 4)
    # ---- what every call was handed
    for i, (name, a, kw, _) in enumerate(calls):
        free_sweep = name in POST and free_name == name and i == len(calls) - 1 and len(sweeps) == 2
        assert a["em"] is em and a["labels"] is lab and a["n_labels"] is n_lab and a["n_frames"] is nf
        if name in POST:
            assert a["onset"] is dp[0] and a["offset"] is dp[1] and a["boundary_window"] == 3 and a["want_gamma"] is False
            assert kw == ([] if name in OLDER_POST else ["boundary_window"])
        else:
            assert kw == []
        if "skip_from" in a:
            if has_spans:
                assert torch.equal(a["skip_from"], skip)
            elif name == PS:                                                # the span sweep without a span: rows of -1
                assert a["skip_from"].shape == (B, L + 1) and a["skip_from"].dtype == torch.int32 and bool((a["skip_from"] == -1).all())
            else:
                assert a["skip_from"] is None
            assert a["skip_penalty"] == 1.5
        if "win_lo" in a:
            if has_win and not free_sweep:
                assert torch.equal(a["win_lo"], win[0]) and torch.equal(a["win_hi"], win[1])
            else:
                assert a["win_lo"] is None and a["win_hi"] is None
        if "repeat_from" in a:
            assert torch.equal(a["repeat_from"], rep) if has_rep else a["repeat_from"] is None
            assert a["repeat_penalty"] == 0.25
        if "path" in a:
            assert a["path"] is (None if free_sweep else dp[4])
    if has_win and free_name not in (None, "log_z"):                        # the free sweep is the last call, and it has no windows
        assert calls[-1][0] == free_name and calls[-1][1].get("win_lo") is None
    # ---- the result: every field is the output of the call the route names for it, or None
    assert isinstance(r, ua.LatticeResult) and r._fields == FIELDS and len(list(r)) == 11
    assert isinstance(r, ua.RepeatLatticeResult) == (dp_name == VR)
    assert all(x is y for x, y in zip(r[:4], dp))
    assert r.path is (dp[4] if dp_name == VR else None)
    post = calls[-len(sweeps)][3] if sweeps else None
    filled = [i < FILLED[kind] for i in range(11)]
    if post_name is None:
        assert (r.visits, r.repeat_count, r.path_prob) == (None, None, None)
    else:
        assert all(x is y for x, y in zip(r[4:8], post[:4]))
        if post_name != P:
            assert r.present_prob is post[5] and r.span_skip_prob is post[6]
        if post_name in (PR, PG):
            assert r.visits is post[5] and r.repeat_count is post[7] and r.path_prob is post[8] and post[8] is not None
        else:
            assert (r.visits, r.repeat_count, r.path_prob) == (None, None, None)
        if kind == "span" or free_name is None:
            assert r.log_z_free is None
        else:
            assert r.log_z_free is (post[3] if free_name == "log_z" else calls[-1][3][3])
            filled[10] = True
    assert [v is not None for v in r] == filled


def test_an_unknown_kind_is_refused_before_any_call(calls):
    from lyricalignment_amd.utils import alignment as ua
    em, lab, n_lab, nf, skip, win, rep = _inputs(3)
    for kind in ("visits", "scored", ""):
        for s, w, rf in ((None, None, None), (skip, win, rep)):
            with pytest.raises(ValueError, match="run_lattice: unknown confidence"):
                ua.run_lattice(em, lab, n_lab, nf, s, w, 1.5, kind, 3, repeat_from=rf)
    assert calls == []
