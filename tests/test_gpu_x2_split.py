"""The operand splits of the f16x2 scheme (csrc/la_x2.h, la_split_f16x2*, la_split_f16x2_t*) against their definition, bit for bit.

The split is exactly defined: the scale s is the power of two that puts the row's largest magnitude in [2^13, 2^14) (1 for an all-zero row),
hi = f16(x s), lo = f16(x s - hi), both round-to-nearest-even with subnormal halves kept; x s and x s - hi are exact in float32.  numpy states
that below; planes, zero padding and inverse scales must equal it in every bit.  (act = "gelu" and the LayerNorm form are not exactly
restatable: tests/test_gpu_finetune.py and tests/test_gpu_x2_inference.py hold them to tolerances.)"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (rows, cols, kp, ldx): the 16-byte path with a zero tail | unaligned rows: the scalar path | the longest row a wave keeps in registers |
# one quad more: the row is read twice
ROW_SHAPES = [(5, 100, 128, 100), (5, 102, 104, 103), (3, 4096, 4096, 4096), (3, 4100, 4104, 4100)]
# (m, k, mp, ldx, one scale from the plain split's maximum): 16-byte column maxima | odd pitch: the scalar pass | no pass at all
T_SHAPES = [(70, 100, 80, 100, False), (70, 99, 80, 99, False), (130, 100, 144, 100, True)]


def _scales(mx):
    """float32 maxima -> (s, 1 / s): s a power of two with mx s in [2^13, 2^14); 1 where mx is 0."""
    mx = mx.astype(np.float32)
    _, e = np.frexp(mx)                                      # mx = m 2^e, m in [0.5, 1)
    sh = np.clip(14 - e, -126, 126)
    ok = (mx > 0) & (mx < 3.0e38)
    one = np.float32(1)
    return np.where(ok, np.ldexp(one, sh), one).astype(np.float32), np.where(ok, np.ldexp(one, -sh), one).astype(np.float32)


def _halves(xs):
    """scaled float32 values -> (hi, lo) float16; numpy's float32 -> float16 conversion rounds to nearest even and keeps subnormals"""
    assert xs.dtype == np.float32
    hi = xs.astype(np.float16)
    return hi, (xs - hi.astype(np.float32)).astype(np.float16)


def _expected(x, scale_of_rows, length):
    """x [r, c] float32, s [r] -> planes [r, 2, length] float16 (zero tail) and what the split stores as inverse scales"""
    s, inv = scale_of_rows
    hi, lo = _halves(x * s[:, None])
    planes = np.zeros((x.shape[0], 2, length), dtype=np.float16)
    planes[:, 0, : x.shape[1]], planes[:, 1, : x.shape[1]] = hi, lo
    return planes, inv


@functools.lru_cache(maxsize=None)
def _operand(rows, cols, seed, spread=60):
    """Normal floats whose row maxima spread over 2^-spread .. 2^spread; row 1 all zero; row 2's elements 2^-20 below its maximum (their lo
    halves are subnormal).  Read-only: shared by the tests."""
    rs = np.random.RandomState(seed)
    x = rs.randn(rows, cols).astype(np.float32)
    x[np.abs(x) < 1e-3] = 1e-3
    x *= np.ldexp(np.float32(1), rs.randint(-spread + 2, spread - 1, size=rows))[:, None].astype(np.float32)
    x[0] *= np.ldexp(np.float32(1), spread) / np.abs(x[0]).max()                         # the two ends of the range are present
    x[rows - 1] *= np.ldexp(np.float32(1), -spread) / np.abs(x[rows - 1]).max()
    x[1] = 0
    x[2, 1:] *= np.float32(2.0 ** -20)
    x[2, 0] = np.abs(x[2, 1:]).max() * np.float32(2.0 ** 20) * np.float32(1.25)
    assert np.isfinite(x).all() and (np.abs(x[x != 0]) > 1e-30).all()
    x.setflags(write=False)
    return x


def _bits(a):
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _pitched(x, ldx):
    """x on the device as a row view of pitch ldx"""
    buf = torch.full((x.shape[0], ldx), 7.0, dtype=torch.float32, device="cuda")
    buf[:, : x.shape[1]] = torch.from_numpy(x.copy())
    return buf[:, : x.shape[1]]


@pytest.mark.parametrize("rows,cols,kp,ldx", ROW_SHAPES)
def test_row_split_equals_its_definition_bit_for_bit(rows, cols, kp, ldx):
    from lyricalignment_amd import f32x2
    x = _operand(rows, cols, 1)
    got = f32x2.split(_pitched(x, ldx), kp)
    planes, inv = _expected(x, _scales(np.abs(x).max(axis=1)), kp)
    assert got.planes.shape == (rows, 2, kp) and got.kp == kp and got.k == cols
    assert np.array_equal(_bits(got.inv_scale.cpu().numpy()), _bits(inv))
    assert np.array_equal(_bits(got.planes.cpu().numpy()), _bits(planes))
    # what the restatement is about: hi + lo carries x s to 22 bits (subnormal lo halves: to 2^-25 of the row's 2^14), and the tail is zero
    assert (planes[:, :, cols:] == 0).all()
    s = _scales(np.abs(x).max(axis=1))[0]
    err = np.abs(planes[:, 0, :cols].astype(np.float64) + planes[:, 1, :cols].astype(np.float64) - x.astype(np.float64) * s[:, None])
    assert (err <= np.maximum(np.abs(x.astype(np.float64) * s[:, None]) * 2.0 ** -22, 2.0 ** -25)).all()


def test_row_split_leaves_the_operand_maximum_in_64_words():
    from lyricalignment_amd import f32x2
    rows, cols = 130, 100
    x = _operand(rows, cols, 2)
    om = f32x2.OperandMax("cuda")
    got = f32x2.split(_pitched(x, cols), 128, omax=om)
    planes, inv = _expected(x, _scales(np.abs(x).max(axis=1)), 128)
    assert np.array_equal(_bits(got.planes.cpu().numpy()), _bits(planes)) and np.array_equal(_bits(got.inv_scale.cpu().numpy()), _bits(inv))
    words = om.words.cpu().numpy().view(np.uint32)
    assert om.valid and om.act is None and words.shape == (64 * 32,)
    row_max = _bits(np.abs(x).max(axis=1))
    want = np.zeros(64 * 32, dtype=np.uint32)
    for r in range(rows):                                   # word (row mod 64), one per 128-byte line: the largest of its rows
        want[(r & 63) * 32] = max(want[(r & 63) * 32], row_max[r])
    assert np.array_equal(words, want)
    assert words.max() == _bits(np.array([np.abs(x).max()], dtype=np.float32))[0]


def _split_t(x, ldx, mp, whole, colsum):
    """f32x2.split_t of x at pitch ldx; whole: with the maximum a plain split of the same operand left (one scale, no pass for column maxima)"""
    from lyricalignment_amd import f32x2
    xd = _pitched(x, ldx)
    om = None
    if whole:
        om = f32x2.OperandMax("cuda")
        f32x2.split(xd, 128, omax=om)
        assert om.valid
    return f32x2.split_t(xd, mp, colsum=colsum, omax=om)


@pytest.mark.parametrize("m,k,mp,ldx,whole", T_SHAPES)
def test_transposed_split_equals_its_definition_bit_for_bit(m, k, mp, ldx, whole):
    # the planes' rows are the operand's columns.  One scale for the whole operand: a spread that keeps the smallest x s a normal float32
    xt = _operand(k, m, 3, 30 if whole else 60)
    x = np.ascontiguousarray(xt.T)
    colsum = torch.full((k,), -7.0, dtype=torch.float32, device="cuda")
    got = _split_t(x, ldx, mp, whole, colsum)
    mx = np.full((k,), np.abs(x).max(), dtype=np.float32) if whole else np.abs(xt).max(axis=1)
    planes, inv = _expected(xt, _scales(mx), mp)
    assert got.planes.shape == (k, 2, mp) and got.rows == k and got.k == m
    assert np.array_equal(_bits(got.inv_scale.cpu().numpy()), _bits(inv))
    assert np.array_equal(_bits(got.planes.cpu().numpy()), _bits(planes))
    # without the column sums the planes are the same
    again = _split_t(x, ldx, mp, whole, None)
    assert torch.equal(again.planes, got.planes) and torch.equal(again.inv_scale, got.inv_scale)
    # The column sums that come out of the same pass, against the float64 sums of the signed values.
    ref, mag = x.astype(np.float64).sum(axis=0), np.abs(x).astype(np.float64).sum(axis=0)
    err = np.abs(colsum.cpu().numpy().astype(np.float64) - ref)
    ulps = err / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    print(f"column sums ({m} x {k}, pitch {ldx}, {'one scale' if whole else 'a scale per column'}): largest error {ulps.max():.3f} ulp, "
          f"{(err / np.maximum(mag, 1e-300)).max() / 2.0 ** -23:.3f} x 2^-23 sum |x|")
    if not whole:
        # a scale per column: the sums come from the pass for column maxima (or la_colsum_f32), float64 partials rounded to float32 once
        assert (ulps <= 1.0).all()
        return
    # One scale: the sums come out of the split kernel itself, which adds four values of a tile in float32 before it goes on in float64
    # (two roundings of 2^-24 each, then the result's own): its error is relative to sum |x|, at most 1.5 x 2^-23 of it, and under
    # cancellation that is many ulps of the signed sum (162 measured on this operand).  One ulp is asked where the two are the same sum:
    # of the operand's magnitudes.
    assert (err <= 1.5 * 2.0 ** -23 * mag).all()
    _split_t(np.abs(x), ldx, mp, whole, colsum)
    ulps = np.abs(colsum.cpu().numpy().astype(np.float64) - mag) / np.spacing(mag.astype(np.float32)).astype(np.float64)
    print(f"column sums of |x|: largest error {ulps.max():.3f} ulp")
    assert (ulps <= 1.0).all()
