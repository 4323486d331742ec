"""CPU-only: gridfour_amd/csrc/gvrs_downsample_common.h, the restatement of the reference's box average that the kernels inline,
compiled with g++ -O2 -ffp-contract=off (tests/csrc/downsample_harness.cpp) and compared BIT FOR BIT with the numpy model of
tests/downsample_ref.py: every factor of the list on blocks whose column count is no multiple of 4 and whose rectangle starts off
the factor's grid; full-mantissa floats with NaN, infinities, -0.0 and subnormals, ints with fills and wrapped sums.  The float
inputs must be able to show a wrong summation order: re-run with the row sums added afterwards, the model differs from the
reference's order in at least one cell in five."""
import numpy as np
import pytest

import downsample_cases as K
import downsample_ref as R


@pytest.fixture(scope="module")
def dh():
    return K.build_harness()


def _block_for(f, k):
    """a rectangle off the factor's grid, a trailing remainder, a column count that is no multiple of 4; some 40 x 60 output cells
    for the small factors, 2 x 3 for f = 67"""
    n_out = (40, 61) if f <= 5 else (12, 19) if f <= 16 else (2, 3)
    row0, col0 = 5 + k, 3 + 2 * k
    n_rows, n_cols = n_out[0] * f + f - 1, n_out[1] * f + f - 1
    if n_cols % 4 == 0:
        n_cols += 1
    return (row0, col0, n_rows, n_cols)


@pytest.mark.parametrize("f", K.FACTORS)
def test_float_harness_equals_model(dh, f):
    rng = np.random.default_rng(1000 + f)
    for k in range(2):
        block = _block_for(f, k)
        assert block[3] % 4 != 0 and (f == 1 or block[0] % f != 0 or block[1] % f != 0)
        v = K.random_floats(rng, block, f)
        want = R.downsample_float(v, block, f)
        assert want.size >= 6 and np.isnan(want).any() and not np.isnan(want).all()
        assert R.same_bits(K.harness_downsample(dh, v, block, f, R.FLOAT, threads=3 * k), want), (f, block)
        if f >= 2:
            # the inputs are not too tame: another summation order shows in at least one cell in five
            plain = rng.uniform(-1000.0, 1000.0, (block[2], block[3])).astype(np.float32)
            a, b = R.downsample_float(plain, block, f), R.downsample_float(plain, block, f, row_sums_first=True)
            share = float((a.view(np.uint32) != b.view(np.uint32)).mean())
            print("f = %d: row sums first differs in %.0f %% of %d cells" % (f, 100 * share, a.size))
            assert share >= 0.2, (f, share)
            assert R.same_bits(K.harness_downsample(dh, plain, block, f, R.FLOAT), a)


@pytest.mark.parametrize("elem_type,fill", [(R.INT, -2 ** 31), (R.INT, 12345), (R.INT, 0), (R.SHORT, -32768), (R.SHORT, 0), (R.SHORT, 32767)])
@pytest.mark.parametrize("f", K.FACTORS)
def test_int_harness_equals_model(dh, f, elem_type, fill):
    rng = np.random.default_rng(2000 + 10 * f + elem_type)
    block = _block_for(f, 1)
    v = K.random_ints(rng, block, f, elem_type, fill)
    want = R.downsample(v, block, f, elem_type, fill)
    assert (want == fill).any() and (want != fill).any()
    assert R.same_bits(K.harness_downsample(dh, v, block, f, elem_type, fill, threads=2), want), (f, elem_type, fill)
    if elem_type == R.INT and f >= 2:
        w = R.windows(v, block, f).astype(np.int64).sum(axis=2)
        assert ((w >= 2 ** 31) | (w < -2 ** 31)).any()                    # sums that wrap are among them


def test_fills_stand_at_every_window_position():
    for f in (2, 3, 4, 5):
        block = _block_for(f, 0)
        v = K.random_ints(np.random.default_rng(5), block, f, R.INT, -7)
        w = R.windows(v, block, f)
        assert ((w == -7).any(axis=(0, 1))).all(), f


def test_axis_rule_equals_model(dh):
    out = np.zeros(2, np.int32)
    for f in (1, 2, 3, 4, 7, 46340):
        for at in (0, 1, 2, 3, 5, 46339, 46340, 2 ** 31 - 100):
            for n in (1, 2, 3, 4, 9, 99):
                dh.dh_axis(at, n, f, out.ctypes.data)
                assert tuple(out) == R.axis(at, n, f), (f, at, n)
