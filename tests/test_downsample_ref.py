"""CPU-only: the numpy model of the reference's ExampleDownsample loop (tests/downsample_ref.py) pinned by answers worked out by
hand from the Java (ExampleDownsample.java:185-206, :228-239)."""
import numpy as np

import downsample_ref as R

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def _one(values, f, elem_type=R.INT, fill=INT_MIN):
    out = R.downsample(np.array(values), (0, 0, f, f), f, elem_type, fill)
    assert out.shape == (1, 1) and out.dtype == R.DTYPES[elem_type]
    return out[0, 0]


def test_integer_averages_round_half_up():
    assert _one([[1, 2], [3, 4]], 2) == 3                                  # 2.5 -> floor(3.0)
    assert _one([[-1, -2], [-3, -4]], 2) == -2                             # -2.5 -> floor(-2.0)
    assert _one([[1, 1, 1], [1, 1, 1], [1, 0, 0]], 3) == 1                 # 7 / 9 = 0.78 -> 1
    assert _one([[-1, -1, -1], [-1, -1, -1], [-1, 0, 0]], 3) == -1         # -0.78 + 0.5 -> floor(-0.28)
    assert _one([[1, 0], [0, 0]], 2) == 0 and _one([[1, 1], [0, 0]], 2) == 1 and _one([[-1, -1], [0, 0]], 2) == 0


def test_integer_sum_wraps_as_a_java_int():
    assert _one([[INT_MAX, 1], [0, 0]], 2) == -536870912                   # the sum is INT_MIN
    assert _one([[INT_MAX, INT_MAX], [2, 0]], 2) == 0                      # 2^32 wraps to 0
    assert _one([[INT_MAX]], 1, fill=0) == INT_MAX
    assert _one([[INT_MIN]], 1, fill=0) == INT_MIN


def test_any_fill_in_the_window_gives_the_fill():
    for k in (0, 4, 8):                                                    # the first, an inner and the last position
        v = np.arange(1, 10)
        v[k] = -999
        assert _one(v.reshape(3, 3), 3, fill=-999) == -999
    assert _one([[INT_MIN]], 1) == INT_MIN
    assert _one([[5, 6], [7, 8]], 2, fill=-999) == 7                       # 6.5 -> 7: no fill, no effect


def test_short():
    assert _one([[-32768, 5], [5, 5]], 2, R.SHORT, -32768) == -32768
    assert _one([[-32768, -32768], [-32768, -32767]], 2, R.SHORT, 0) == -32768     # -32767.75 + 0.5 -> floor
    assert _one([[0, 5], [5, 5]], 2, R.SHORT, 0) == 0                      # a fill of 0
    assert _one([[32767, 32767], [32767, 32767]], 2, R.SHORT, -32768) == 32767
    assert _one([[1, 2], [3, 4]], 2, R.SHORT, -32768) == 3


def test_float_sums_in_sequence():
    assert _one([[1e8, 1.0], [-1e8, 1.0]], 2, R.FLOAT) == np.float32(0.25)  # ((1e8 + 1) - 1e8) + 1 = 1, not 2
    assert _one([[1e8, -1e8], [1.0, 1.0]], 2, R.FLOAT) == np.float32(0.5)
    z = R.downsample(np.array([[-0.0]], np.float32), (0, 0, 1, 1), 1, R.FLOAT)
    assert z[0, 0] == 0.0 and not np.signbit(z[0, 0])                      # 0.0f + -0.0f
    assert np.isnan(_one([[np.inf, 1.0], [1.0, -np.inf]], 2, R.FLOAT))
    assert _one([[np.inf, 1.0], [1.0, 1.0]], 2, R.FLOAT) == np.inf
    assert np.isnan(_one([[np.nan, 1.0], [1.0, 1.0]], 2, R.FLOAT))         # a NaN fill propagates
    tiny = np.float32(1e-45)
    assert _one([[tiny, tiny], [tiny, tiny]], 2, R.FLOAT) == tiny          # 4 ulp / 4, subnormal throughout
    assert _one([[tiny * 3, tiny * 3], [tiny, tiny * 5]], 2, R.FLOAT) == tiny * 3
    assert _one([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.5]], 3, R.FLOAT) == np.float32(45.5) / np.float32(9.0)


def test_row_sums_first_is_another_order():
    v = np.array([[1.0, 1e8], [-1e8, 1.0]])
    assert _one(v, 2, R.FLOAT) == np.float32(0.25)                         # ((1 + 1e8) - 1e8) + 1 = 1: the 1 is lost once
    assert R.downsample_float(v, (0, 0, 2, 2), 2, row_sums_first=True)[0, 0] == np.float32(0.0)   # (1 + 1e8) + (-1e8 + 1) = 0


def test_rectangle_rule():
    assert R.out_rect((0, 0, 10, 10), 2) == (0, 0, 5, 5)
    assert R.out_rect((0, 0, 11, 13), 3) == (0, 0, 3, 4)                    # trailing remainder ignored
    assert R.out_rect((1, 2, 10, 10), 3) == (1, 1, 2, 3)                    # rows 3..8 of 1..10; columns 3..11 of 2..11
    assert R.out_rect((3, 6, 3, 3), 3) == (1, 2, 1, 1)
    assert R.out_rect((4, 4, 4, 4), 3)[2:] == (0, 0)                        # rows 4..7 hold no whole window: 6..8 ends outside
    assert R.out_rect((1, 0, 2, 9), 3)[2] == 0                              # empty
    assert R.out_rect((5, 5, 1, 1), 1) == (5, 5, 1, 1)
    assert R.out_rect((0, 0, 5, 5), 6) == (0, 0, 0, 0)
    # strips tile the whole: the cells of [0, 100) by 7 come from strips of 13 rows exactly once
    whole = R.axis(0, 100, 7)
    got = []
    for at in range(0, 100, 13):
        first, n = R.axis(at, min(13, 100 - at), 7)
        got += list(range(first, first + n))
    # (a window that straddles two strips belongs to neither: the caller overlaps its strips by f - 1 rows)
    assert set(got) <= set(range(whole[0], whole[0] + whole[1]))
    got = []
    for at in range(0, 100, 14):                                            # strips that start on multiples of 7 lose nothing
        first, n = R.axis(at, min(14, 100 - at), 7)
        got += list(range(first, first + n))
    assert got == list(range(whole[0], whole[0] + whole[1]))


def test_windows_of_a_block_off_the_grid_of_the_factor():
    v = np.arange(7 * 9).reshape(7, 9)
    out = R.downsample(v, (2, 1, 7, 9), 3, R.INT, -1)                       # rows 2..8, columns 1..9: windows at rows 3, 6; columns 3, 6
    assert out.shape == (2, 2)
    assert out[0, 0] == v[1:4, 2:5].sum() // 9 + (1 if (v[1:4, 2:5].sum() % 9) * 2 >= 9 else 0)
    assert out[1, 1] == int(np.floor(v[4:7, 5:8].sum() / 9.0 + 0.5))
