"""Host side of the per-clip (ragged-batch) mode, no GPU: frame counts, the harness's bookkeeping with a stub model, and the
argument validation of the three C entry points (la_logmel_ragged_f32_prepared, la_gru_layer_ragged, la_align_head_forward_ragged)."""
import ctypes

import numpy as np
import pytest
import torch


def test_per_clip_frame_counts_follow_frame_plan():
    """T_b = int(round(n_mel_b / 2.0)), Python's banker's rounding, for lengths around the rounding cases."""
    from lyricalignment_amd.module.align_model import frame_plan
    from oracle import model_oracle as mo
    want = {0: 0, 1: 0, 2: 1, 3: 2, 5: 2, 7: 4, 300: 150, 301: 150, 302: 151, 303: 152, 2999: 1500, 3000: 1500}
    for n_mel, T in want.items():
        assert frame_plan(n_mel, True) == [(0, n_mel, T)]
        assert mo.frame_count(n_mel) == T
    # the six clips of tests/test_gpu_ragged.py
    assert [frame_plan(n // 160, True)[0][2] for n in (60096, 24237, 101760, 48160, 480000, 9000)] == [188, 76, 318, 150, 1500, 28]
    from lyricalignment_amd import harness
    assert harness.PER_CLIP_MAX_SAMPLES // 160 == 3000 and (harness.PER_CLIP_MAX_SAMPLES + 1) // 160 == 3001


class _StubModel:
    """AlignModel.align's contract on the host: clip -> boundaries that depend on the clip alone (its length and labels), so that any
    mix-up of order, labels or routing shows.  Records every call."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _one(audio, labs):
        base = len(audio) / 16000.0
        return [[base + 0.02 * j + 0.001 * int(c), base + 0.02 * j + 0.01 + 0.001 * int(c)] for j, c in enumerate(labs)]

    def align(self, audios, labels, use_ctc=True, per_clip=False, return_confidence=False, **kw):
        assert not kw, kw
        rows = [[int(v) for v in row if int(v) != -100] for row in (labels.tolist() if torch.is_tensor(labels) else labels)]
        assert len(rows) == len(audios)
        self.calls.append(dict(n=len(audios), per_clip=per_clip, lens=[len(a) for a in audios]))
        if not per_clip:
            assert len(audios) == 1                    # (this stub does not model the reference's batch coupling)
        res = [self._one(a, r) for a, r in zip(audios, rows)]
        if return_confidence:
            return res, [{"occupancy": [0.5 + 0.01 * j for j in range(len(r))]} for r in rows]
        return res


class _Rec:
    def __init__(self, audio, text):
        self.audio, self.text = audio, text


def _records():
    rs = np.random.RandomState(3)
    lens = [48000, 9000, 480159, 16000, 480160, 32000, 700000, 20000, 8000]      # two records of more than 30 s (3001 mel frames and more)
    texts = ["".join(chr(0x4E00 + 11 * i + j) for j in range(2 + i % 4)) for i in range(len(lens))]
    ids = {t: [int(v) for v in rs.randint(1, 50, size=len(t))] for t in texts}
    return [_Rec(np.zeros(n, np.float32), t) for n, t in zip(lens, texts)], ids


def test_align_records_batching_restores_order_and_routes_long_records_alone():
    from lyricalignment_amd.harness import PinyinClassLUT, align_records
    lut = PinyinClassLUT([str(i) for i in range(60)], {str(i): (i * 7) % 60 for i in range(60)})
    records, ids = _records()
    one = _StubModel()
    want = align_records(one, records, lut, lambda t: ids[t], batch_size=1)
    assert [c["n"] for c in one.calls] == [1] * len(records) and not any(c["per_clip"] for c in one.calls)
    assert [[e[2] for e in r] for r in want] == [list(r.text) for r in records]
    for bs in (2, 4, 32):
        m = _StubModel()
        got = align_records(m, records, lut, lambda t: ids[t], batch_size=bs)
        assert got == want, bs
        long_calls = [c for c in m.calls if not c["per_clip"]]
        assert sorted(c["lens"][0] for c in long_calls) == [480160, 700000] and all(c["n"] == 1 for c in long_calls)
        batched = [c for c in m.calls if c["per_clip"]]
        assert [c["n"] for c in batched] == [min(bs, 7 - k) for k in range(0, 7, bs)]
        flat = [n for c in batched for n in c["lens"]]
        assert flat == sorted(flat) and max(flat) == 480159                   # sorted by length; 3000 mel frames still go batched
    m = _StubModel()
    conf = align_records(m, records, lut, lambda t: ids[t], with_confidence=True, batch_size=4)
    conf1 = align_records(_StubModel(), records, lut, lambda t: ids[t], with_confidence=True, batch_size=1)
    assert conf == conf1 and [[e[:3] for e in r] for r in conf] == want
    with pytest.raises(ValueError):
        align_records(m, records, lut, lambda t: ids[t], batch_size=0)


def _batches():
    rs = np.random.RandomState(5)
    out = []
    for i in range(11):
        n = int(rs.randint(8000, 120000))
        L = int(rs.randint(1, 6))
        tokens = torch.full((1, 6), -100, dtype=torch.long)
        tokens[0, :L] = torch.from_numpy(rs.randint(1, 50, size=L))
        gt = (None,) if i in (2, 7) else [[[float(rs.rand()), float(rs.rand()) + 1.0] for _ in range(L)]]
        out.append(([np.zeros(n, np.float32)], tokens, None, gt, None, None))
    return out


def test_evaluate_batches_group_keeps_per_batch_maes_and_their_mean():
    from lyricalignment_amd.harness import PinyinClassLUT, evaluate_batches
    lut = PinyinClassLUT([str(i) for i in range(60)], {str(i): (i * 7) % 60 for i in range(60)})
    batches = _batches()
    m1 = _StubModel()
    avg1, maes1 = evaluate_batches(m1, batches, lut, use_ctc_loss=True)
    assert maes1[2] is None and maes1[7] is None and sum(v is not None for v in maes1) == 9
    assert [c["n"] for c in m1.calls] == [1] * 9
    m4 = _StubModel()
    avg4, maes4 = evaluate_batches(m4, batches, lut, use_ctc_loss=True, group=4)
    assert maes4 == maes1 and avg4 == avg1                                    # exactly: same per-batch values, same accumulation order
    assert [c["n"] for c in m4.calls] == [4, 4, 1] and all(c["per_clip"] for c in m4.calls)
    # a clip of more than 30 s inside a grouped run goes alone through the dense call, the rest still in groups
    long = list(batches)
    long[4] = ([np.zeros(490000, np.float32)],) + tuple(batches[4][1:])
    a1, v1 = evaluate_batches(_StubModel(), long, lut, group=1)
    mg = _StubModel()
    a4, v4 = evaluate_batches(mg, long, lut, group=4)
    assert v4 == v1 and a4 == a1
    assert [(c["n"], c["per_clip"]) for c in mg.calls] == [(1, False), (4, True), (4, True)]
    # what grouping does not define
    two = list(batches)
    two[1] = ([np.zeros(9000, np.float32), np.zeros(9000, np.float32)],) + tuple(batches[1][1:])
    with pytest.raises(ValueError):
        evaluate_batches(_StubModel(), two, lut, group=4)
    with pytest.raises(ValueError):
        evaluate_batches(_StubModel(), batches, lut, group=0)
    with pytest.raises(ValueError):
        evaluate_batches(_StubModel(), batches, lut, group=2, two_step=True)


def test_ragged_entry_points_validate_on_the_host():
    """Rejected before any HIP call, in the style of test_argument_validation_without_gpu: null length arrays, lengths the host can see are
    inconsistent (out_frames below max_samples / 160), fewer than 201 samples."""
    from lyricalignment_amd import _lib
    L = _lib.lib()
    P = 256                                                           # a non-null, 256-byte aligned stand-in pointer
    need = ctypes.c_size_t(0)
    # ---- log-mel
    assert L.la_logmel_ragged_workspace_bytes(6, 480000, ctypes.byref(need)) == _lib.LA_OK
    dense = ctypes.c_size_t(0)
    assert L.la_logmel_workspace_bytes(6, 480000, ctypes.byref(dense)) == _lib.LA_OK and need.value == dense.value
    assert L.la_logmel_ragged_workspace_bytes(0, 480000, ctypes.byref(need)) == _lib.LA_EINVAL
    ok = (P, P, 6, 480000, P, P, 80 * 3000, 3000, 3000, P, 1 << 40, 0)
    bad = lambda i, v: ok[:i] + (v,) + ok[i + 1:]
    assert L.la_logmel_ragged_f32_prepared(*bad(1, 0)) == _lib.LA_EINVAL and "n_samples" in _lib.last_error()
    assert L.la_logmel_ragged_f32_prepared(*bad(4, 0)) == _lib.LA_EINVAL and "constants" in _lib.last_error()
    assert L.la_logmel_ragged_f32_prepared(*bad(3, 200)) == _lib.LA_EINVAL and "200 samples" in _lib.last_error()
    assert L.la_logmel_ragged_f32_prepared(*bad(8, 2999)) == _lib.LA_EINVAL and "out_frames" in _lib.last_error()
    assert L.la_logmel_ragged_f32_prepared(*bad(7, 2999)) == _lib.LA_EINVAL                                        # row stride < out_frames
    assert L.la_logmel_ragged_f32_prepared(*bad(10, 16)) == _lib.LA_EINVAL and "workspace too small" in _lib.last_error()
    # ---- recurrence
    assert L.la_gru_workspace_bytes(6, 1500, 384, ctypes.byref(need)) == _lib.LA_OK
    gru_ok = (_lib.LA_BF16, P, P, P, P, 0, 6, 1500, P, 384, P, need.value, 0, 0)
    gbad = lambda i, v: gru_ok[:i] + (v,) + gru_ok[i + 1:]
    assert L.la_gru_layer_ragged(*gbad(8, 0)) == _lib.LA_EINVAL and "n_frames" in _lib.last_error()
    assert L.la_gru_layer_ragged(*gbad(11, 16)) == _lib.LA_EINVAL and "workspace too small" in _lib.last_error()
    assert L.la_gru_layer_ragged(*gbad(9, 100)) == _lib.LA_EUNSUPPORTED                                            # hidden % 64
    assert L.la_gru_layer_ragged(*gbad(6, 0)) == _lib.LA_OK                                                        # an empty batch is a no-op, as la_gru_layer's
    # ---- head
    V2 = ctypes.c_void_p * 2
    hw = _lib.HeadWeightsC(_lib.LA_BF16, 384, 1024, 21129, 2, V2(P, P), V2(P, P), V2(P, P), V2(P, P), P, P)
    head = lambda nf, ws: L.la_align_head_forward_ragged(ctypes.byref(hw), P, 1024, 1500, 6, 1500, nf, 1, P, 26, P, 26, P, P, 26, P, P, 0, P, ws, 0, 0)
    assert head(0, 1 << 40) == _lib.LA_EINVAL and "n_frames" in _lib.last_error()
    assert head(P, 16) == _lib.LA_EINVAL and "workspace too small" in _lib.last_error()
    # ---- the Python wrappers refuse what only the host can see
    from lyricalignment_amd.utils import alignment as ua
    if not torch.cuda.is_available():
        return
    with pytest.raises(ValueError):
        ua.perform_viterbi_ctc(torch.zeros(2, 10, 8), torch.tensor([[1, 2], [2, 3]]), n_frames=[10, 11])          # a length above Tmax
    with pytest.raises(ValueError):
        ua.perform_viterbi_ctc(torch.zeros(2, 10, 8), torch.tensor([[1, 2], [2, 3]]), n_frames=[10])
