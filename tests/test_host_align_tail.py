"""utils.alignment.align_labels, the one tail behind perform_viterbi* and AlignModel.align, without a GPU: a fake emissions_of and the
recorders of tests/test_host_lattice_routes.py (plus two for the readings' fold and scores).  For every combination of {no confidence,
a scored kind, a repeat kind} x return_segments x {no alternatives, alternatives, alternatives + return_readings}: the shape of the
return value (bare, or a tuple whose elements come in the order seconds, segments, scores, readings), that emissions_of is asked once
-- for the expanded labels exactly when alternatives are given --, and the errors raised before anything is launched."""
import pytest
import torch

from test_host_lattice_routes import B, T, VR, calls  # noqa: F401  (calls: the recorder fixture)

HOP = 0.02
LISTS = [[3, 5, 3], [4, 6]]
ALTERNATIVES = [[(1, [7, 8])], []]
REPEAT_SPANS = [[(0, 2)], []]
SEGMENTS_ERROR = "repeat_spans / return_segments do not go with a confidence"


@pytest.fixture
def readings_calls(monkeypatch):
    from lyricalignment_amd import ops
    log = []

    def merge_readings(em_x, alt_start, n_labels, n_frames, out=None):
        log.append(("merge_readings", em_x))
        return torch.zeros((em_x.shape[0], em_x.shape[1], alt_start.shape[1]))

    def reading_scores(em_x, alt_start, n_labels, onset, offset):
        log.append(("reading_scores", em_x, onset, offset))
        return torch.zeros(onset.shape, dtype=torch.int32), torch.zeros((em_x.shape[0], em_x.shape[2] - 1), dtype=torch.float64)
    monkeypatch.setattr(ops, "merge_readings", merge_readings)
    monkeypatch.setattr(ops, "reading_scores", reading_scores)
    return log


def _labels():
    lab = torch.zeros((B, 3), dtype=torch.int32)
    for b, l in enumerate(LISTS):
        lab[b, : len(l)] = torch.tensor(l, dtype=torch.int32)
    return lab, torch.tensor([len(l) for l in LISTS], dtype=torch.int32)


class _Emissions:
    """emissions_of: records what it is asked and answers zeros; fused: it also has a DP result, and leaves the emissions out where they
    are not needed (the fused head of AlignModel.align)."""

    def __init__(self, fused=False):
        self.asked, self.fused = [], fused
        self.dp = (torch.full((B, 3), 4, dtype=torch.int32), torch.full((B, 3), 5, dtype=torch.int32), torch.zeros((B,), dtype=torch.float64),
                   torch.zeros((B,), dtype=torch.int32))

    def __call__(self, lab, n_lab, needed=True):
        self.asked.append((lab, n_lab, needed))
        em = torch.zeros((B, T, lab.shape[1] + 1)) if needed or not self.fused else None
        return (self.dp if self.fused else None), em


def _tail(emissions_of, confidence, return_segments, alternatives, return_readings, repeat_spans=None, raw=False):
    from lyricalignment_amd.utils import alignment as ua
    lab, n_lab = _labels()
    out = ua.align_labels("perform_viterbi", emissions_of, lab, n_lab, LISTS, [T] * B, T, None, HOP, confidence, 2, None, None, 0.0, None,
                          repeat_spans, 0.0, return_segments, alternatives, return_readings, raw=raw)
    return out, lab


@pytest.mark.parametrize("readings", ["no_alternatives", "alternatives", "return_readings"])
@pytest.mark.parametrize("return_segments", [False, True], ids=["", "segments"])
@pytest.mark.parametrize("confidence", [None, "anchored", "song"])
def test_the_shape_of_the_return_value_and_what_emissions_of_is_asked(calls, readings_calls, confidence, return_segments, readings):  # noqa: F811
    from lyricalignment_amd.utils import alignment as ua
    alternatives = None if readings == "no_alternatives" else ALTERNATIVES
    emissions_of = _Emissions()
    if confidence == "anchored" and return_segments:                       # no segments with an older confidence: before anything is asked
        with pytest.raises(ValueError, match=SEGMENTS_ERROR):
            _tail(emissions_of, confidence, True, alternatives, readings == "return_readings")
        assert emissions_of.asked == [] and calls == [] and readings_calls == []
        return
    out, lab = _tail(emissions_of, confidence, return_segments, alternatives, readings == "return_readings")
    # ---- emissions_of: once; for the labels themselves, or with alternatives for the expanded rows (and never for the labels)
    assert len(emissions_of.asked) == 1
    asked_lab, asked_n, needed = emissions_of.asked[0]
    if alternatives is None:
        assert asked_lab is lab and needed == (confidence is not None or return_segments)
        assert readings_calls == []
    else:
        rd = ua._readings_of(ALTERNATIVES, LISTS)
        assert torch.equal(asked_lab, rd.labels_x) and asked_lab.shape == (B, 5) and asked_n.tolist() == [5, 2] and needed is True
        assert [c[0] for c in readings_calls] == ["merge_readings"] + ["reading_scores"] * (readings == "return_readings")
        assert calls[0][1]["em"] is not readings_calls[0][1] and torch.equal(calls[0][1]["labels"], rd.lattice_ids)     # the folded matrix, the set ids
    # ---- the lattice calls: the route of the kind (a path for the segments comes from the lattice with repeatable spans)
    names = [c[0] for c in calls]
    assert names == {None: [VR] if return_segments else ["viterbi_batch"], "anchored": ["viterbi_batch", "alignment_posteriors_spans"],
                     "song": [VR, "alignment_posteriors_song"]}[confidence]
    # ---- the return value: seconds [, segments] [, scores] [, readings], bare when seconds is all there is
    want = ["seconds"] + ["segments"] * return_segments + ["scores"] * (confidence is not None) + ["readings"] * (readings == "return_readings")
    if want == ["seconds"]:
        out = (out,)
    assert isinstance(out, tuple) and len(out) == len(want)
    for name, value in zip(want, out):
        assert isinstance(value, list) and len(value) == B, name
        if name == "seconds":
            assert value == [[[0.0, HOP]] * len(l) for l in LISTS]
        elif name == "segments":
            assert value == [[(0, 0.0, T * HOP)]] * B                      # the recorder's path: state 1 at every frame
        elif name == "scores":
            keys = {"occupancy", "onset_prob", "offset_prob", "path_log_posterior", "span_skip_prob"}
            keys |= {"sung_prob", "window_log_prob"} if confidence == "anchored" else {"visits", "repeat_count", "visit_occupancy"}
            assert all(isinstance(d, dict) and set(d) == keys for d in value)
        else:
            assert value == [[(3, [0.0]), (5, [0.0, 0.0, 0.0]), (3, [0.0])], [(4, [0.0]), (6, [0.0])]]


def test_repeat_spans_and_the_fused_shortcut(calls, readings_calls):  # noqa: F811
    from lyricalignment_amd.utils import alignment as ua
    # repeat spans with an older confidence: refused like the segments; with a repeat kind and on their own they reach the DP
    with pytest.raises(ValueError, match=SEGMENTS_ERROR):
        _tail(_Emissions(), "sheet", False, None, False, repeat_spans=REPEAT_SPANS)
    assert calls == []
    for confidence in (None, "repeat"):
        del calls[:]
        _tail(_Emissions(), confidence, False, None, False, repeat_spans=REPEAT_SPANS)
        assert calls[0][0] == VR and calls[0][1]["repeat_from"].tolist() == [[2, -1, -1], [-1, -1, -1]]
    # the repeat kind stops at 511 labels, before anything is asked; the song kind does not
    wide, emissions_of = torch.ones((1, 512), dtype=torch.int32), _Emissions()
    with pytest.raises(NotImplementedError, match="perform_viterbi_repeat_scored: 512 labels exceed the 511-label limit"):
        ua.align_labels("perform_viterbi", emissions_of, wide, torch.tensor([512], dtype=torch.int32), [[1] * 512], [T], T, None, HOP, "repeat", 2,
                        None, None, 0.0, None, None, 0.0, False, None, False)
    assert emissions_of.asked == []
    # a provider with the plain lattice's DP (the fused head): no confidence, no face -> its result, emissions not needed, NO lattice call
    del calls[:]
    fused = _Emissions(fused=True)
    (r, picked), lab = _tail(fused, None, False, None, False, raw=True)
    assert calls == [] and picked == () and type(r) is ua.LatticeResult and all(a is b for a, b in zip(r[:4], fused.dp)) and list(r[4:]) == [None] * 7
    assert [(a[0] is lab, a[2]) for a in fused.asked] == [(True, False)]
    out, _ = _tail(fused, None, False, None, False)
    assert out == [[[4 * HOP, 5 * HOP]] * len(l) for l in LISTS] and calls == []
    # with a confidence its DP is handed to run_lattice, which takes it where the route's DP is the plain lattice's
    (r, picked), _ = _tail(fused, "plain", False, None, False, raw=True)
    assert [c[0] for c in calls] == ["alignment_posteriors"] and calls[0][1]["onset"] is fused.dp[0] and r.onset is fused.dp[0]
    # raw with readings: ops.reading_scores' pair behind the result
    (r, picked), _ = _tail(_Emissions(), None, False, ALTERNATIVES, True, raw=True)
    assert len(picked) == 2 and picked[0].shape == (B, 3) and picked[1].shape == (B, 5) and readings_calls[-1][2] is r.onset


def test_return_readings_without_alternatives_is_refused_first():
    from lyricalignment_amd.module.align_model import AlignModel
    from lyricalignment_amd.utils import alignment as ua
    for fn in (ua.perform_viterbi, ua.perform_viterbi_ctc_scored, ua.perform_viterbi_song_scored):
        with pytest.raises(ValueError, match="^return_readings goes with alternatives"):
            fn(None, None, return_readings=True)                            # before the prediction is looked at
    with pytest.raises(ValueError, match="^align: return_readings goes with alternatives"):
        AlignModel.align(AlignModel.__new__(AlignModel), [None], [[1, 2]], return_readings=True)     # before the model is looked at
