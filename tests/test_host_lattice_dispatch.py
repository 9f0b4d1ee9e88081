"""utils.alignment.run_lattice without a GPU: with the six ops.* lattice calls replaced by recorders, the calls it makes for every
(confidence, spans, windows) are the row of tests/test_gpu_lattice_dispatch.py's DISPATCH table, in order and with the DP's frames, the
spans, the windows and the penalty handed on; the result carries each call's outputs in the fields of LatticeResult."""
import pytest
import torch

from test_gpu_lattice_dispatch import DISPATCH, FIELDS

B, T, L = 2, 6, 3
DP = ("viterbi_batch", "viterbi_spans_batch", "viterbi_windows_batch")
POST = ("alignment_posteriors", "alignment_posteriors_spans", "alignment_posteriors_windows")


@pytest.fixture
def calls(monkeypatch):
    from lyricalignment_amd import ops
    log = []

    def recorder(name):
        def call(*args, **kw):
            assert not kw
            log.append((name, args))
            tag = float(len(log))
            if name in DP:
                return tuple(torch.full((B, L), tag + i / 8) for i in range(2)) + tuple(torch.full((B,), tag + i / 8) for i in (2, 3))
            out = tuple(torch.full((B, L), tag + i / 8) for i in range(3)) + (torch.full((B,), tag + 0.375), torch.full((B,), tag + 0.5))
            return out if name == "alignment_posteriors" else out + (torch.full((B, L), tag + 0.625), torch.full((B, L + 1), tag + 0.75))
        return call
    for name in DP + POST:
        monkeypatch.setattr(ops, name, recorder(name))
    return log


@pytest.mark.parametrize("key", list(DISPATCH), ids=[f"{c}-spans{int(s)}-windows{int(w)}" for c, s, w in DISPATCH])
@pytest.mark.parametrize("head_dp", [False, True])
def test_run_lattice_makes_the_calls_of_the_dispatch_table(calls, key, head_dp):
    from lyricalignment_amd.utils import alignment as ua
    conf, has_spans, has_win = key
    dp_name, post_name, free_name = DISPATCH[key]
    em, lab = torch.zeros((B, T, L + 1)), torch.ones((B, L), dtype=torch.int32)
    n_lab, nf = torch.full((B,), L, dtype=torch.int32), torch.full((B,), T, dtype=torch.int32)
    skip = torch.full((B, L + 1), -1, dtype=torch.int32)
    skip[0, 2] = 0
    win = (torch.zeros((B, 2 * L + 1), dtype=torch.int32), torch.full((B, 2 * L + 1), T, dtype=torch.int32))
    given = tuple(torch.full(s, 9.0) for s in ((B, L), (B, L), (B,), (B,)))
    r = ua.run_lattice(em, lab, n_lab, nf, skip if has_spans else None, win if has_win else None, 1.5, conf, 3, dp=given if head_dp else None)
    assert isinstance(r, ua.LatticeResult) and r._fields == FIELDS
    takes_given = head_dp and dp_name == "viterbi_batch"                    # a DP result that exists is the plain lattice's only
    want = ([] if takes_given else [dp_name]) + [n for n in (post_name, free_name) if n not in (None, "log_z")]
    assert [name for name, _ in calls] == want
    dp = given if takes_given else r[:4]
    assert all(torch.equal(a, b) for a, b in zip(r[:4], given)) == takes_given
    for name, args in calls:
        assert all(a is b for a, b in zip(args[:4], (em, lab, n_lab, nf)))
        rest = list(args[4:])
        if name in POST:
            assert rest[0] is dp[0] and rest[1] is dp[1] and rest[-1] == 3    # the reported path and boundary_window
            rest = rest[2:-1]
        if "windows" in name:
            assert torch.equal(rest[0], win[0]) and torch.equal(rest[1], win[1])
            rest = rest[2:]
        if name not in ("viterbi_batch", "alignment_posteriors"):
            if has_spans:
                assert torch.equal(rest[0], skip)
            else:                                                            # no span: None on the window face, all -1 on the span face
                assert rest[0] is None if "windows" in name else bool((rest[0] == -1).all()) and rest[0].shape == (B, L + 1)
            assert rest[1] == 1.5
    # every field is the output of the call the table names for it, or None
    n_dp = 0 if takes_given else 1
    filled = {None: 4, "plain": 8, "span": 10, "anchored": 11}[conf]
    assert [v is not None for v in r] == [i < filled for i in range(11)]
    if post_name is not None:
        tag = n_dp + 1.0
        assert [float(t.flatten()[0]) for t in r[4:8]] == [tag, tag + 0.125, tag + 0.25, tag + 0.375]
        if conf != "plain":
            assert float(r.present_prob[0, 0]) == tag + 0.625 and float(r.span_skip_prob[0, 0]) == tag + 0.75
        if conf == "anchored":
            assert float(r.log_z_free[0]) == (tag if free_name == "log_z" else tag + 1) + 0.375
