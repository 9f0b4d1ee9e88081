"""Pronunciation alternatives on the device (csrc/la_readings.hip: la_emissions_merge_readings folds the expanded emission matrix into the
merged classes in front of the lattice, la_reading_scores names the reading that was sung behind it) and the layers over them
(ops.merge_readings / ops.reading_scores, the `alternatives` / `return_readings` keywords of perform_viterbi(_ctc) and AlignModel.align,
harness.align_song(heteronyms=...)).

Yardstick: readings_reference (float64 numpy), and for the lattice repeat_spans_reference.viterbi run on the device's folded matrix.

Bound of the fold, derived and never measured: column 0 and single-reading columns are copies, so bit-equal.  A merged column is the
float32 rounding of m + log(sum exp(x_a - m)) evaluated in float64 on both sides; the two float64 values differ by a few float64 ulps (exp
and log of two libraries, at most 8 addends), and rounding two values that close lands on the same float32 or, when a rounding boundary
lies between them, on neighbouring ones: equal or adjacent float32, nothing wider.  The share that is exactly equal is printed.
The segment sums are sequential float64 additions of the same float32 inputs in the same order: bit-equal."""
import functools

import numpy as np
import pytest
import torch

import readings_reference as rdr
import repeat_spans_reference as rr
from test_gpu_repeat_spans import PEN, RPEN, _planted_logits, make_clip
from test_gpu_wide_posteriors import _score_differences
from test_gpu_windows import _windows_around

pytestmark = pytest.mark.gpu

HOP = 0.02
SENT = -77.25                                     # what the outputs hold before a call: no emission, score or reading of a case equals it


def _mixed_counts(seed, L, threes, twos):
    counts = np.array([3] * threes + [2] * twos + [1] * (L - threes - twos))
    return [int(v) for v in np.random.RandomState(seed).permutation(counts)]


CASES = {
    # ragged n_labels and n_frames inside a batch, 1 .. 3 readings per position
    "B3_T37_L5": dict(T=[37, 20, 31], counts=[[1, 2, 3, 1, 2], [2, 1, 3], [3, 3, 1, 2]]),
    "B1_T9_L1_A8": dict(T=[9], counts=[[8]]),
    # expanded widths 257 and 258: groups straddle the 64-lane and 256-thread edges
    "B2_T130_L100_X257_X258": dict(T=[130, 97], counts=[_mixed_counts(1, 100, 57, 43), _mixed_counts(2, 100, 58, 42)]),
    # 2047 two-reading positions: 4095 expanded columns
    "B1_T50_L2048_X4095": dict(T=[50], counts=[[2] * 2047 + [1]]),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> list of clips: dict(T, L, alt [L+1], em_x [T, X+1] float32, onset, offset [L]) with the reference results ref64 / ref32 [T, L+1],
    col_score [X], reading [L], computed once on the host and left unchanged."""
    spec = CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    clips = []
    for T, counts in zip(spec["T"], spec["counts"]):
        L = len(counts)
        alt = [0] + [int(v) for v in np.cumsum(counts)]
        X = alt[-1]
        em_x = (-rs.rand(T, X + 1) * 12.0).astype(np.float32)
        multi = [n for n in range(L) if counts[n] > 1]
        for i, n in enumerate(multi):                                  # the values the issue names, each on about half of the frames
            rows = np.flatnonzero(rs.rand(T) < 0.5)
            g = slice(1 + alt[n], 1 + alt[n + 1])
            kind = i % 6
            if kind == 0:
                em_x[rows, 1 + alt[n]] = -1000.0                       # one reading at the emission floor
            elif kind == 1:
                em_x[rows, g] = -np.inf                                # every reading impossible
            elif kind == 2:
                em_x[rows, alt[n + 1]] = -np.inf                       # the last reading impossible
            elif kind == 3:
                em_x[rows, g] = em_x[rows, 1 + alt[n]][:, None]        # equal readings
            elif kind == 4:
                em_x[rows, g] = -92.0                                  # a spread of 90 between the readings
                em_x[rows, 1 + alt[n]] = -2.0
            else:
                em_x[rows, g] = -1000.0                                # every reading at the floor
        em_x[0, 0] = -1000.0
        # segments: any [onset, offset) inside the clip; position 0 one frame long, position 1 the whole clip, every fifth one skipped
        onset = [int(rs.randint(0, T)) for _ in range(L)]
        offset = [int(rs.randint(t + 1, T + 1)) for t in onset]
        onset[0], offset[0] = T // 2, T // 2 + 1
        onset[min(1, L - 1)], offset[min(1, L - 1)] = 0, T
        for n in range(4, L, 5):
            onset[n] = offset[n] = -1
        tie = next((n for n in multi if onset[n] >= 0), None)           # an exact tie: two identical columns, the others far below
        if tie is not None:
            em_x[:, 1 + alt[tie]: 1 + alt[tie + 1]] = em_x[:, 1 + alt[tie] + 1][:, None] - 50.0
            em_x[:, 1 + alt[tie]] = em_x[:, 1 + alt[tie] + 1] = (-rs.rand(T) * 5.0).astype(np.float32)
        ref64 = rdr.fold_rows64(em_x, alt)
        col_score = rdr.segment_scores(em_x, alt, onset, offset)
        reading = rdr.pick_readings(col_score, alt, onset)
        if tie is not None:
            assert reading[tie] == 0 and col_score[alt[tie]] == col_score[alt[tie] + 1]
        clips.append(dict(T=T, L=L, alt=alt, counts=counts, em_x=em_x, onset=onset, offset=offset, ref64=ref64, ref32=ref64.astype(np.float32),
                          col_score=col_score, reading=reading, tie=tie))
    return clips


def _device_inputs(clips):
    """The clips of one launch, padded: em_x with an ODD row stride behind a one-element offset (no row start is 16-byte aligned) and NaN
    wherever the kernels must not read; alt_start rows padded with the last value."""
    B = len(clips)
    Tmax, Lmax, Xmax = max(c["T"] for c in clips), max(c["L"] for c in clips), max(c["alt"][-1] for c in clips)
    XS = (Xmax + 1) | 1
    flat = torch.full((B * Tmax * XS + 1,), float("nan"), dtype=torch.float32)
    em_x = flat[1:].view(B, Tmax, XS)[:, :, : Xmax + 1]
    alt = torch.zeros((B, Lmax + 1), dtype=torch.int32)
    on = torch.full((B, Lmax), -1, dtype=torch.int32)
    off = torch.full((B, Lmax), -1, dtype=torch.int32)
    for b, c in enumerate(clips):
        em_x[b, : c["T"], : c["alt"][-1] + 1] = torch.from_numpy(c["em_x"])
        alt[b] = torch.tensor(c["alt"] + [c["alt"][-1]] * (Lmax - c["L"]), dtype=torch.int32)
        on[b, : c["L"]] = torch.tensor(c["onset"], dtype=torch.int32)
        off[b, : c["L"]] = torch.tensor(c["offset"], dtype=torch.int32)
    em_x = flat.cuda()[1:].view(B, Tmax, XS)[:, :, : Xmax + 1]
    assert em_x.data_ptr() % 16 != 0 and (em_x.stride(1) * 4) % 16 != 0
    n_lab = torch.tensor([c["L"] for c in clips], dtype=torch.int32).cuda()
    nf = torch.tensor([c["T"] for c in clips], dtype=torch.int32).cuda()
    return em_x, alt.cuda(), n_lab, nf, on.cuda(), off.cuda(), (B, Tmax, Lmax, Xmax)


def _merge(clips):
    """-> the whole output buffer [B, Tmax, Lmax + 4] (row stride wider than Lmax + 1), pre-filled with SENT."""
    from lyricalignment_amd import ops
    em_x, alt, n_lab, nf, _, _, (B, Tmax, Lmax, _) = _device_inputs(clips)
    out = torch.full((B, Tmax, Lmax + 4), SENT, dtype=torch.float32, device="cuda")
    assert ops.merge_readings(em_x, alt, n_lab, nf, out=out) is out
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _scores(clips):
    """la_reading_scores on pre-filled outputs wider than needed -> reading [B, Lmax + 2] (-9 before), col_score [B, Xmax + 3] (SENT)."""
    from lyricalignment_amd import _lib, ops
    em_x, alt, n_lab, _, on, off, (B, Tmax, Lmax, Xmax) = _device_inputs(clips)
    reading = torch.full((B, Lmax + 2), -9, dtype=torch.int32, device="cuda")
    col = torch.full((B, Xmax + 3), SENT, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().la_reading_scores(em_x.data_ptr(), em_x.stride(0), em_x.stride(1), alt.data_ptr(), alt.stride(0), n_lab.data_ptr(),
                                            on.data_ptr(), off.data_ptr(), Lmax, B, Tmax, Lmax, Xmax, col.data_ptr(), Xmax + 3,
                                            reading.data_ptr(), Lmax + 2, _lib.stream_ptr()), "reading_scores")
    r2, c2 = ops.reading_scores(em_x, alt, n_lab, on, off)             # the wrapper: the same numbers in its own tensors
    torch.cuda.synchronize()
    reading, col, r2, c2 = (t.cpu().numpy() for t in (reading, col, r2, c2))
    for b, c in enumerate(clips):
        assert r2[b, : c["L"]].tolist() == reading[b, : c["L"]].tolist()
        assert c2[b, : c["alt"][-1]].tobytes() == col[b, : c["alt"][-1]].tobytes()
    return reading, col


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the fold
@pytest.mark.parametrize("name", list(CASES))
def test_the_fold_equals_the_float64_reference(name):
    clips = case(name)
    out = _merge(clips)
    exact = total = 0
    for b, c in enumerate(clips):
        T, L, alt = c["T"], c["L"], c["alt"]
        got = out[b, :T, : L + 1]
        assert (_bits(got[:, 0]) == _bits(c["em_x"][:, 0])).all(), (name, b, "silence")
        for n in range(L):
            col, ref = got[:, 1 + n], c["ref32"][:, 1 + n]
            if c["counts"][n] == 1:
                assert (_bits(col) == _bits(c["em_x"][:, 1 + alt[n]])).all(), (name, b, n, "a single reading is a copy")
                continue
            same = col == ref
            near = (col == np.nextafter(ref, np.float32(np.inf))) | (col == np.nextafter(ref, np.float32(-np.inf)))
            assert (same | near).all(), (name, b, n, col[~(same | near)], ref[~(same | near)])
            assert not np.isnan(col).any()
            exact += int(same.sum()); total += T
        # everything outside [0, L_b] x [0, T_b) still holds the sentinel: later rows, later columns, the stride padding
        assert (out[b, T:, :] == SENT).all() and (out[b, :, L + 1:] == SENT).all(), (name, b)
        assert np.isneginf(c["ref32"]).any() or name == "B1_T9_L1_A8"
    print(f"{name}: merged values exactly equal to the rounded float64 reference: {exact} of {total} ({100.0 * exact / total:.3f} %)")


@pytest.mark.parametrize("name", ["B3_T37_L5", "B2_T130_L100_X257_X258"])
def test_a_clip_alone_equals_the_clip_in_a_batch_and_two_calls_agree(name):
    clips = case(name)
    first, second = _merge(clips), _merge(clips)
    assert first.tobytes() == second.tobytes()
    r1, s1 = _scores(clips)
    r2, s2 = _scores(clips)
    assert r1.tobytes() == r2.tobytes() and s1.tobytes() == s2.tobytes()
    for b, c in enumerate(clips):
        alone = _merge([c])
        assert alone[0, : c["T"], : c["L"] + 1].tobytes() == first[b, : c["T"], : c["L"] + 1].tobytes(), (name, b)
        ra, sa = _scores([c])
        assert ra[0, : c["L"]].tolist() == r1[b, : c["L"]].tolist() and sa[0, : c["alt"][-1]].tobytes() == s1[b, : c["alt"][-1]].tobytes()


# ------------------------------------------------------------------------------------------------ 2. the reading scores
@pytest.mark.parametrize("name", list(CASES))
def test_reading_scores_equal_the_reference_bit_for_bit(name):
    clips = case(name)
    reading, col = _scores(clips)
    for b, c in enumerate(clips):
        L, X = c["L"], c["alt"][-1]
        assert col[b, :X].tobytes() == c["col_score"].tobytes(), (name, b)
        assert reading[b, :L].tolist() == c["reading"], (name, b)
        assert (reading[b, L:] == -9).all() and (col[b, X:] == SENT).all(), (name, b, "beyond the clip's labels / columns: untouched")
        for n in range(L):                                             # a skipped position: reading -1, scores 0
            if c["onset"][n] < 0:
                assert reading[b, n] == -1 and (col[b, c["alt"][n]: c["alt"][n + 1]] == 0.0).all()
        if c["tie"] is not None:                                       # the smallest index wins an exact tie
            j = c["alt"][c["tie"]]
            assert col[b, j] == col[b, j + 1] and reading[b, c["tie"]] == 0
    lengths = {o - t for c in clips for t, o in zip(c["onset"], c["offset"]) if t >= 0}
    assert (1 in lengths or name == "B1_T9_L1_A8") and any(o - t == c["T"] for c in clips for t, o in zip(c["onset"], c["offset"]))
    assert any(r > 0 for c in clips for r in c["reading"]) or max(c["L"] for c in clips) < 10      # (the wide cases: not only reading 0 wins)


# ------------------------------------------------------------------------------------------------ 3. the lattice on the folded matrix
@functools.lru_cache(maxsize=None)
def lattice_case(T, L):
    """A planted clip of test_gpu_repeat_spans (one repeatable line sung twice, one optional line left out) whose every third position
    has two or three readings: the planted column's probability split among them, so the fold gives the planted matrix back up to
    rounding.  One pair of neighbours has EQUAL reading sets (the equal-neighbour rule through a set id)."""
    from lyricalignment_amd.utils import alignment as ua
    c = make_clip(1000 + L, T, L, "both")
    rs = np.random.RandomState(L)
    lab = [int(v) for v in c["lab"]]
    counts = [1 + (n % 3 == 1) + (n % 7 == 3) for n in range(L)]
    counts[L // 2 - 1] = counts[L // 2] = 2                            # _labels made these two neighbours equal: equal sets as well
    assert lab[L // 2 - 1] == lab[L // 2]
    sets = [[lab[n]] + [2000 + 3 * lab[n] + k for k in range(counts[n] - 1)] for n in range(L)]
    alternatives = [[(n, r[1:]) for n, r in enumerate(sets) if len(r) > 1]]
    rd = ua._readings_of(alternatives, [lab])
    ids = rdr.lattice_ids(sets)
    assert rd.lattice_ids[0].tolist() == ids and ids[L // 2 - 1] == ids[L // 2] >= rdr.READING_SET_ID and rd.n_columns == [sum(counts)]
    em_x = np.empty((T, sum(counts) + 1), dtype=np.float32)
    em_x[:, 0] = c["em"][:, 0]
    alt = rd.alt_start[0].tolist()
    for n in range(L):
        w = rs.dirichlet(np.ones(counts[n]))
        em_x[:, 1 + alt[n]: 1 + alt[n + 1]] = c["em"][:, 1 + n][:, None] + np.log(w)[None, :].astype(np.float32)
    return dict(c=c, rd=rd, ids=ids, em_x=em_x)


@pytest.mark.parametrize("T,L", [(90, 26), (160, 100), (700, 600)])       # <= 64 states; several waves; the strip kernel
def test_the_lattice_on_the_folded_matrix_equals_the_float64_restatements(T, L):
    from lyricalignment_amd import ops
    from lyricalignment_amd.utils import alignment as ua
    k = lattice_case(T, L)
    c, rd, ids = k["c"], k["rd"], k["ids"]
    assert c["skip"] is not None and c["rf"] is not None
    em_x = torch.from_numpy(k["em_x"])[None].cuda()
    n_lab = torch.tensor([L], dtype=torch.int32).cuda()
    nf = torch.tensor([T], dtype=torch.int32).cuda()
    em = ops.merge_readings(em_x, rd.alt_start.cuda(), n_lab, nf)
    folded = em[0].cpu().numpy()                                         # the device's folded matrix is the reference's input
    ids_dev = rd.lattice_ids.cuda()
    skip = torch.tensor([c["skip"]], dtype=torch.int32)
    rf = torch.tensor([c["rf"]], dtype=torch.int32)
    plain = rr.viterbi(folded, ids, rows=True)
    lo, hi = _windows_around(np.random.RandomState(T), plain[4], 2 * L + 1, T)
    win = (torch.tensor([lo], dtype=torch.int32), torch.tensor([hi], dtype=torch.int32))
    faces = {"plain": (dict(), plain),
             "optional_spans": (dict(skip_from=skip, skip_penalty=PEN), rr.viterbi(folded, ids, c["skip"], PEN, rows=True)),
             "windows": (dict(windows=win), rr.viterbi(folded, ids, lo=lo, hi=hi, rows=True)),
             "repeat_spans": (dict(skip_from=skip, skip_penalty=PEN, repeat_from=rf, repeat_penalty=RPEN),
                              rr.viterbi(folded, ids, c["skip"], PEN, c["rf"], RPEN, rows=True))}
    assert faces["repeat_spans"][1].n_repeats > 0 and faces["optional_spans"][1][0] != plain[0]
    for face, (kw, ref) in faces.items():
        r = ua.run_lattice(em, ids_dev, n_lab, nf, **kw)
        on, off, st = r.onset.cpu().numpy(), r.offset.cpu().numpy(), r.status.cpu().numpy()
        print(f"T={T} L={L} {face}: status {st[0]} / {ref[3]}, score {float(r.score[0])!r} / {ref[2]!r}")
        assert st[0] == ref[3] == rr.LA_OK and on[0].tolist() == ref[0] and off[0].tolist() == ref[1], (T, L, face)
    # the reading scores on the repeat lattice's boundaries: the reported (first) visit
    r = ua.run_lattice(em, ids_dev, n_lab, nf, **faces["repeat_spans"][0])
    reading, col = ops.reading_scores(em_x, rd.alt_start.cuda(), n_lab, r.onset, r.offset)
    ref = faces["repeat_spans"][1]
    want = rdr.segment_scores(k["em_x"], rd.alt_start[0].tolist(), ref[0], ref[1])
    assert col[0].cpu().numpy().tobytes() == want.tobytes()
    assert reading[0].tolist() == rdr.pick_readings(want, rd.alt_start[0].tolist(), ref[0]) and -1 in reading[0].tolist()


# ------------------------------------------------------------------------------------------------ 4. planted logits
def test_a_character_sung_with_its_other_reading_on_planted_logits():
    from lyricalignment_amd.utils import alignment as ua
    labels = torch.tensor([[4, 3, 9, 6]])                              # the sheet says 3 where the audio sings 7
    sung = [4, 7, 9, 6]
    lg = _planted_logits(sung, 5 * (2 * len(sung) + 1), 12, 5).cuda()
    planted = [(5 + 10 * i, 10 + 10 * i) for i in range(4)]
    plain = ua.perform_viterbi_ctc(lg, labels)
    assert [(round(a / HOP), round(b / HOP)) for a, b in plain[0]][1] != planted[1]          # without alternatives the character is misplaced
    seconds, readings = ua.perform_viterbi_ctc(lg, labels, alternatives=[[(1, [7])]], return_readings=True)
    assert [(round(a / HOP), round(b / HOP)) for a, b in seconds[0]] == planted
    assert seconds == ua.perform_viterbi_ctc(lg, labels, alternatives=[[(1, [7])]])
    cls, scores = readings[0][1]
    assert cls == 7 and len(scores) == 2 and scores[1] > scores[0]
    assert [r[0] for r in readings[0]] == [4, 7, 9, 6] and all(len(r[1]) == 1 for i, r in enumerate(readings[0]) if i != 1)
    # the sheet's own class wins where it was sung: the extra reading changes nothing there
    sec2, rd2 = ua.perform_viterbi_ctc(lg, labels, alternatives=[[(1, [7]), (2, [5])]], return_readings=True)
    assert sec2 == seconds and rd2[0][2][0] == 9 and rd2[0][2][1][0] > rd2[0][2][1][1]
    # an extra class outside the range has the floor everywhere: the result of the plain call
    assert ua.perform_viterbi_ctc(lg, labels, alternatives=[[(1, [500])]]) == plain
    # None and all-empty: the call as it was; a skipped character has no reading
    assert ua.perform_viterbi_ctc(lg, labels, alternatives=None) == plain and ua.perform_viterbi_ctc(lg, labels, alternatives=[[]]) == plain
    same, trivial = ua.perform_viterbi_ctc(lg, labels, alternatives=[[]], return_readings=True)
    assert same == plain and [r[0] for r in trivial[0]] == [4, 3, 9, 6]
    lg5 = _planted_logits([4, 7, 6], 5 * 7, 12, 5).cuda()               # the line "9" is not sung
    sec5, rd5 = ua.perform_viterbi_ctc(lg5, labels, alternatives=[[(1, [7])]], optional_spans=[[(2, 3)]], return_readings=True)
    assert sec5[0][2] is None and rd5[0][2] is None and rd5[0][1][0] == 7
    for bad in ([[(4, [7])]], [[(1, [3])]], [[(1, [])]], [[(1, [7]), (1, [8])]], [[], []]):
        with pytest.raises(ValueError):
            ua.perform_viterbi_ctc(lg, labels, alternatives=bad)


# ------------------------------------------------------------------------------------------------ 5. the model
@pytest.fixture(scope="module")
def tiny():
    import test_gpu_ragged as tr
    from test_gpu_parity_full import _build
    model, _ = _build("tiny", torch.float32)
    idx = [0, 1, 3, 5]                                           # clips of tests/test_gpu_ragged.py: 11, 5, 8, 3 labels
    labels = tr._padded_labels(idx)

    def extras(b, n, k):
        v = int(labels[b, n])
        return [(v + 17) % 400 + 2, (v + 101) % 400 + 2][:k]

    alts = [[(0, extras(0, 0, 1)), (4, extras(0, 4, 2)), (10, extras(0, 10, 1))], [(2, extras(1, 2, 2))], [], [(1, extras(3, 1, 1))]]
    return dict(model=model, audios=[tr._clip(i) for i in idx], labels=labels, tr=tr, idx=idx, alts=alts)


# every emission of the fused head and of the two-step route lies within 1e-3 of the float64 oracle (tests/test_gpu_model.py), so within
# 2e-3 of each other: a segment score of n frames within 2e-3 n, and the two routes name the same reading wherever the best score leads
# the second by more than twice that
EM_TOL = 2e-3


def _assert_same_readings(fused, two, seconds):
    for b, (rf, rt) in enumerate(zip(fused, two)):
        for n, (x, y) in enumerate(zip(rf, rt)):
            assert (x is None) == (y is None) == (seconds[b][n] is None)
            if x is None:
                continue
            frames = round((seconds[b][n][1] - seconds[b][n][0]) / HOP)
            assert len(x[1]) == len(y[1]) and all(abs(p - q) <= EM_TOL * frames for p, q in zip(x[1], y[1])), (b, n, x, y)
            top = sorted(x[1], reverse=True)
            if len(top) == 1 or top[0] - top[1] > 2 * EM_TOL * frames:
                assert x[0] == y[0], (b, n, x, y)


@pytest.mark.parametrize("use_ctc", [True, False])
def test_align_with_alternatives_equals_the_two_step_route(tiny, use_ctc):
    from lyricalignment_amd.utils import alignment as ua
    model, audios, labels, alts = tiny["model"], tiny["audios"], tiny["labels"], tiny["alts"]
    two = ua.perform_viterbi_ctc if use_ctc else ua.perform_viterbi
    sheet = ua.perform_viterbi_ctc_sheet_scored if use_ctc else ua.perform_viterbi_sheet_scored
    with torch.no_grad():
        logits, _ = model.frame_manual_forward(audios)
        plain = model.align(audios, labels, use_ctc=use_ctc)
        for kw in (dict(), dict(optional_spans=[[(7, 9)], [], [(5, 8)], []], skip_penalty=0.5), dict(onset_anchors=[[(4, 1.0, 0.5)], [], [], []]),
                   dict(repeat_spans=[[(3, 7), (0, 2)], [(0, 5)], [(2, 3)], []], return_segments=True)):
            fused = model.align(audios, labels, use_ctc=use_ctc, alternatives=alts, return_readings=True, **kw)
            other = two(logits, labels, alternatives=alts, return_readings=True, **kw)
            assert len(fused) == len(other) == (3 if "return_segments" in kw else 2)
            assert fused[:-1] == other[:-1], kw                                     # seconds (and segments): the same frames
            _assert_same_readings(fused[-1], other[-1], fused[0])
            without = model.align(audios, labels, use_ctc=use_ctc, alternatives=alts, **kw)
            assert without == (fused[0] if len(fused) == 2 else fused[:-1])
            frames = model.align(audios, labels, use_ctc=use_ctc, alternatives=alts, return_readings=True, return_frames=True, **kw)
            assert len(frames) == (7 if "return_segments" in kw else 6)
            reading, col = frames[-2], frames[-1]
            assert reading.dtype == torch.int32 and reading.shape == (4, 11) and col.dtype == torch.float64 and col.shape == (4, 15)
            for b, row in enumerate(fused[-1]):                                     # the lists are the tensors
                for n, r in enumerate(row):
                    assert (r is None) == (int(reading[b, n]) < 0)
        print(f"use_ctc={use_ctc}: readings of clip 0 {[r and r[0] for r in fused[-1][0]]} for labels {labels[0].tolist()}")
        # with a confidence: the posteriors of the merged class, on both routes
        f_sec, f_sc, f_rd = model.align(audios, labels, use_ctc=use_ctc, alternatives=alts, return_readings=True, return_sheet_confidence=True)
        t_sec, t_sc, t_rd = sheet(logits, labels, alternatives=alts, return_readings=True)
        assert f_sec == t_sec
        _assert_same_readings(f_rd, t_rd, f_sec)
        T = logits.shape[1]                                       # the two routes' scores: the bound of tests/test_gpu_wide_posteriors.py
        for a, b in zip(f_sc, t_sc):
            diff, d_w = _score_differences(a, b)
            print(f"use_ctc={use_ctc}: fused against the two-step sheet scores {diff}")
            assert all(x <= 8 * T * 2.0 ** -23 for x in diff.values()) and d_w <= 16 * T * 2.0 ** -23, diff
        # None and all-empty: today's call
        assert model.align(audios, labels, use_ctc=use_ctc, alternatives=None) == plain
        assert model.align(audios, labels, use_ctc=use_ctc, alternatives=[[], [], [], []]) == plain
        a = model.align(audios, labels, use_ctc=use_ctc, return_frames=True)
        b = model.align(audios, labels, use_ctc=use_ctc, alternatives=[[], [], [], []], return_frames=True)
        assert len(a) == len(b) == 4 and all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))


def test_per_clip_the_long_form_and_the_sheet_functions_with_alternatives(tiny):
    from lyricalignment_amd.harness import PinyinClassLUT, align_song
    from lyricalignment_amd.utils import alignment as ua
    from test_gpu_parity_full import VOCAB
    model, audios, labels, tr, alts = tiny["model"], tiny["audios"], tiny["labels"], tiny["tr"], tiny["alts"]
    with torch.no_grad():
        batch = model.align(audios, labels, per_clip=True, alternatives=alts, return_readings=True)
        for r, i in enumerate(tiny["idx"]):
            alone = model.align([audios[r]], tr._clip_labels(i), per_clip=True, alternatives=[alts[r]], return_readings=True)
            assert batch[0][r] == alone[0][0], i                                   # each clip as if alone: the same frames
            _assert_same_readings([batch[1][r]], alone[1], [batch[0][r]])          # (the head's emissions may differ in their last bits
                                                                                   # between batch sizes: its GEMM is routed by its row count)
        audio = np.concatenate([tr._clip(4), tr._clip(3)])                               # 33 s: two encoder chunks
        lab = torch.from_numpy(np.random.RandomState(5).randint(2, 403, size=(1, 14)))
        kw = dict(alternatives=[[(2, [int(lab[0, 2]) % 400 + 3]), (9, [int(lab[0, 9]) % 400 + 3, 405])]], optional_spans=[[(10, 14)]])
        logits, _ = model.frame_manual_forward([audio])
        assert logits.shape[1] > 1500
        fused = model.align([audio], lab, return_readings=True, **kw)
        other = ua.perform_viterbi_ctc(logits, lab, return_readings=True, **kw)
        assert fused[0] == other[0]
        _assert_same_readings(fused[1], other[1], fused[0])
        # one whole-sheet call: every character entry names the class that was sung
        lut = PinyinClassLUT([str(i) for i in range(VOCAB)], {str(i): i for i in range(VOCAB)})       # token id -> the same class id
        ids_all = [int(v) for v in tr._clip_labels(0)[0]]                                             # 11 labels: lines of 3 / 4 / 2 / 2
        lines = ["".join(chr(0x4E00 + 11 * k + j) for j in range(n)) for k, n in enumerate((3, 4, 2, 2))]
        ids, pos = {}, 0
        for line in lines:
            ids[line] = ids_all[pos: pos + len(line)]
            pos += len(line)
        heteronyms = {ids_all[0]: [str(alts[0][0][1][0])], ids_all[4]: [str(c) for c in alts[0][1][1]]}
        got, conf = align_song(model, tr._clip(0), lines, lut, lambda t: ids[t], heteronyms=heteronyms)
        old, conf_old = align_song(model, tr._clip(0), lines, lut, lambda t: ids[t])
        assert [len(e) for line in old for e in line] == [3] * 11 and [len(e) for line in got for e in line] == [4] * 11
        flat = [e for line in got for e in line]
        assert all(e[3] == ids_all[n] for n, e in enumerate(flat) if ids_all[n] not in heteronyms)
        assert flat[0][3] in (ids_all[0], alts[0][0][1][0]) and flat[4][3] in [ids_all[4]] + alts[0][1][1]
        assert set(conf) == set(conf_old)
