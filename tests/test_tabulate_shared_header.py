"""CPU-only: gridfour_amd/csrc/gvrs_tabulate_common.h, the restatement of the reference's data assessment that the kernels inline,
compiled with g++ -O2 -ffp-contract=off (tests/csrc/tabulate_harness.cpp) and compared BIT FOR BIT with the numpy model of
tests/tabulate_ref.py on the same inputs: Java's (int) cast at its edges, the plan arithmetic with a wrapped difference and a
saturated product, the per-sample index rule on every element type with the reference's traps among the inputs, the (value, index)
ordering with its ties and its two zeroes, one thread and several, one call and three accumulated strips."""
import numpy as np
import pytest

import tabulate_cases as K
import tabulate_ref as R


@pytest.fixture(scope="module")
def th():
    return K.build_harness()


def _same(got, want):
    return np.array_equal(got[0], want[0]) and R.same_summary(got[1], want[1])


def test_java_int_equals_model(th):
    xs = [0.0, -0.0, 0.5, -0.5, 0.99, -0.99, 1.5, -1.5, 2 ** 31 - 1.5, 2 ** 31 - 1.0, 2 ** 31 - 0.5, 2.0 ** 31, -2.0 ** 31, -2.0 ** 31 - 0.5,
          -2.0 ** 31 - 1.0, 1e20, -1e20, np.inf, -np.inf, np.nan, -10999.9, -11000.1, 4.99999988, 5.0]
    want = R.java_int(xs)
    assert [th.th_java_int(x) for x in xs] == want.tolist()
    assert want[[9, 11, 12, 14, 19, 20, 21]].tolist() == [2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, -2 ** 31, 0, -10999, -11000]


def test_plan_equals_model(th):
    for def_min, def_max, scale in [K.REF_RANGE, (0, 99, 0.9), (-50, 60, 0.7), (10, 300, 0.35), (-2 ** 31, 2 ** 31 - 1, 1.0), (0, 2 ** 31 - 2, 4.0),
                                    (-7, -7, 1.0), (0, -1, 1.0), (-1000, 1000, 1e-3), (5, 2 ** 31 - 1, 0.5), (-2 ** 30, 0, 3.0), (3, 9, 1e300)]:
        want = R.plan(def_min, def_max, scale)
        assert want is not None and K.harness_plan(th, def_min, def_max, scale) == want, (def_min, def_max, scale)
    assert K.harness_plan(th, -2 ** 31, 2 ** 31 - 2, 1.0)["n_counter"] == -1 and K.harness_plan(th, 0, 10, float("nan"))["n_counter"] == 0


def test_sample_and_index_equal_model(th):
    """the sample of a value through the FP64 form, of an int cell at scale 1 through the form without FP64 (the kernels' choice when
    scale_used is 1.0: both must give the model's sample on every int), and the one-comparison index rule"""
    rng = np.random.default_rng(12)
    ints = np.concatenate([np.array([-2 ** 31, -2 ** 31 + 1, -32769, -32768, -3, -2, -1, 0, 1, 2, 3, 32767, 32768, 2 ** 31 - 2, 2 ** 31 - 1], np.int64),
                           rng.integers(-2 ** 31, 2 ** 31, 3000), rng.integers(-40, 41, 300)])
    want = R.samples_of(ints, 1.0)
    assert [th.th_sample_unit(int(v)) for v in ints] == want.tolist() == [th.th_sample(float(v), 1.0) for v in ints]
    assert want[:8].tolist() == [-2 ** 31 + 1, -2 ** 31 + 2, -32768, -32767, -2, -1, 0, 0]
    for scale in (0.9, 0.35, 2.5, 1e-3):
        su = float(np.float32(scale))
        assert [th.th_sample(float(v), su) for v in ints[:400]] == R.samples_of(ints[:400], su).tolist()
    for base, n_counter in ((-11000, 19651), (2 ** 31 - 100, 300), (-2 ** 31, 0), (5, 2 ** 31 - 1), (0, 0)):
        for sample in (base, base - 1, base + 1, _w32(base + n_counter), _w32(base + n_counter + 1), -2 ** 31, 2 ** 31 - 1, 0, -1):
            index = _w32(sample - base)
            assert th.th_index(sample, base, n_counter) == (-1 if index < 0 or index > n_counter else index), (sample, base, n_counter)


def _w32(x):
    return (x + 2 ** 31) % 2 ** 32 - 2 ** 31


def test_symbols_equal_model(th):
    v = np.array([0, 1, -1, -32768, 32767, 255, -256], np.int16)
    assert [th.th_symbol_i16(int(x)) for x in v] == R.keys_of(v, R.SHORT).tolist()
    w = np.array([0, 1, -1, -2 ** 31, 2 ** 31 - 1], np.int32)
    assert [th.th_symbol_i32(int(x)) for x in w] == R.keys_of(w, R.INT).tolist()


@pytest.mark.parametrize("elem_type", [R.INT, R.SHORT, R.FLOAT])
def test_dense_harness_equals_model(th, elem_type):
    rng = np.random.default_rng(300 + elem_type)
    for k, (lo, hi, scale) in enumerate([K.REF_RANGE, (-50, 60, 0.9), (10, 300, 0.35), (-7, -7, 1.0), (0, -1, 1.0), (-300, 500, 2.5)]):
        v = K.dem_like(rng, 5000 + 13 * k, elem_type, lo, hi)
        if elem_type != R.FLOAT:
            v[rng.random(v.size) < 0.05] = -7
        for skip in (False, True):
            for threads in (0, 3):
                got = K.harness_dense(th, v, elem_type, lo, hi, scale, fill_i=-7, skip_fill=skip, first_cell=77 * k, threads=threads)
                assert _same(got, R.dense(v, elem_type, lo, hi, scale, fill_i=-7, skip_fill=skip, first_cell=77 * k)), (elem_type, k, skip, threads)


def test_dense_harness_on_the_traps(th):
    v = K.scale_trap_block()
    for scale in (0.9, 0.7, 0.35):
        want = R.dense(v, R.INT, 0, int(v.max()), scale)
        assert _same(K.harness_dense(th, v, R.INT, 0, int(v.max()), scale), want)
        assert not np.array_equal(want[0], R.dense(v, R.INT, 0, int(v.max()), scale, scale_used=scale)[0])      # the double would differ
    for v in K.zero_blocks() + (K.float_edge_block(), np.full(9, np.nan, np.float32), np.zeros(0, np.float32)):
        for threads in (0, 2):
            assert _same(K.harness_dense(th, v, R.FLOAT, *K.REF_RANGE, threads=threads), R.dense(v, R.FLOAT, *K.REF_RANGE)), v
    # samples below, above and wrapping around the window: base = 2^31 - 100, and a sample near -2^31 lands inside it
    w = np.array([2 ** 31 - 100, 2 ** 31 - 1, 2 ** 31 - 101, -2 ** 31 + 5, -2 ** 31 + 300, 0], np.int32)
    want = R.dense(w, R.INT, 2 ** 31 - 100, 2 ** 31 - 1, 1.0)
    assert want[0][0] == 1 and want[0][99] == 1 and want[0][100] == 0 and want[0].sum() == 2 and want[1]["n_samples"] == 2
    assert _same(K.harness_dense(th, w, R.INT, 2 ** 31 - 100, 2 ** 31 - 1, 1.0), want)


def test_dense_harness_accumulates(th):
    rng = np.random.default_rng(6)
    for elem_type in (R.INT, R.FLOAT):
        v = K.dem_like(rng, 3000, elem_type)
        ext = np.nanmin(v) - 1
        v[[10, 1400, 2850]] = ext                                          # a tie across the strips
        whole = R.dense(v, elem_type, *K.REF_RANGE)
        for order in (((0, 1000), (1000, 2000), (2000, 3000)), ((2000, 3000), (0, 1000), (1000, 2000))):
            acc = None
            for a, b in order:
                acc = K.harness_dense(th, v[a:b], elem_type, *K.REF_RANGE, first_cell=a, into=acc)
            assert _same(acc, whole) and acc[1]["min_at"] == 10, (elem_type, order)
