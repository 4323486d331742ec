"""CPU-only: the numpy model of the block tabulation (tests/tabulate_ref.py) against a literal cell-by-cell transcription of the
Java loops on small inputs, and the reference's traps -- each a way to get the feature wrong -- present in the test inputs and
visible in the model: the float the collector's constructor keeps its scale in, Java's truncating cast beside the window's ends,
infinities and NaN, negative symbols behind the positive ones, the two zeroes of a FLOAT minimum."""
import math

import numpy as np
import pytest

import tabulate_cases as K
import tabulate_ref as R


def _same_dense(a, b):
    return np.array_equal(a[0], b[0]) and R.same_summary(a[1], b[1]) and R.same_summary(b[1], a[1])


@pytest.mark.parametrize("elem_type", [R.INT, R.SHORT, R.FLOAT])
def test_dense_model_equals_the_literal_loops(elem_type):
    rng = np.random.default_rng(100 + elem_type)
    outside = 0
    for k, (lo, hi, scale) in enumerate([K.REF_RANGE, (-50, 60, 0.9), (10, 300, 0.35), (-7, -7, 1.0), (0, -1, 1.0), (-300, 500, 2.5)]):
        v = K.dem_like(rng, 700, elem_type, lo, hi)
        if elem_type != R.FLOAT:
            v[rng.random(v.size) < 0.05] = -7
        for skip in (False, True):
            got = R.dense(v, elem_type, lo, hi, scale, fill_i=-7, skip_fill=skip, first_cell=1000 * k)
            want = R.dense_literal(v, elem_type, lo, hi, scale, fill_i=-7, skip_fill=skip, first_cell=1000 * k)
            assert _same_dense(got, want), (elem_type, lo, hi, scale, skip)
            outside += got[1]["n_samples"] < got[1]["n_cells"] - got[1]["n_skipped"]
    assert outside >= 4                                                    # samples fall outside the window in some of the cases
    for v in K.zero_blocks() + (K.float_edge_block(),):
        if elem_type == R.FLOAT:
            assert _same_dense(R.dense(v, R.FLOAT, *K.REF_RANGE), R.dense_literal(v, R.FLOAT, *K.REF_RANGE))


def test_dense_model_accumulates_as_one_call():
    rng = np.random.default_rng(5)
    v = K.dem_like(rng, 900, R.INT)
    v[[10, 400, 850]] = v.min() - 1                                        # the same minimum in all three strips
    whole = R.dense(v, R.INT, *K.REF_RANGE)
    acc = None
    for a, b in ((0, 300), (300, 600), (600, 900)):
        acc = R.dense(v[a:b], R.INT, *K.REF_RANGE, first_cell=a, into=acc)
    assert _same_dense(acc, whole) and whole[1]["min_at"] == 10
    back = None
    for a, b in ((600, 900), (300, 600), (0, 300)):                        # a tie goes to the smaller global index in any order
        back = R.dense(v[a:b], R.INT, *K.REF_RANGE, first_cell=a, into=back)
    assert _same_dense(back, whole)


@pytest.mark.parametrize("elem_type", [R.INT, R.SHORT, R.FLOAT])
def test_symbol_model_equals_the_literal_loops(elem_type):
    rng = np.random.default_rng(200 + elem_type)
    v = K.dem_like(rng, 1500, elem_type, -200, 300)
    got, want = R.symbols(v, elem_type), R.symbols_literal(v, elem_type)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert got[2]["n_unique"] > 0 and got[2]["n_repeated"] > 0 and got[2]["max_count"] > 1


@pytest.mark.parametrize("scale", [0.9, 0.7, 0.35])
def test_trap_the_scale_went_through_a_float(scale):
    v = K.scale_trap_block()
    as_float, as_double = R.samples_of(v, np.float32(scale)), R.samples_of(v, scale)
    assert (as_float != as_double).any(), scale
    hi = int(v.max())
    a, b = R.dense(v, R.INT, 0, hi, scale), R.dense(v, R.INT, 0, hi, scale, scale_used=scale)
    assert not np.array_equal(a[0], b[0])
    if scale == 0.9:
        assert R.samples_of([5], np.float32(0.9))[0] == 4 and R.samples_of([5], 0.9)[0] == 5       # 5 * 0.9f + 0.5 = 4.99999988


def test_trap_the_window_ends_and_what_touches_no_counter():
    v = K.float_edge_block()
    counter, s = R.dense(v, R.FLOAT, *K.REF_RANGE)
    p = R.plan(*K.REF_RANGE)
    assert (p["n_counter"], p["base"], p["n_bins"]) == (19651, -11000, 19652)
    index = R.samples_of(v[5:9], 1.0).astype(np.int64) - p["base"]
    # (int) truncates toward zero: -11000.4 + 0.5 = -10999.9 -> -10999, -11000.6 + 0.5 = -11000.1 -> -11000
    assert index.tolist() == [19650, 19651, 1, 0]
    for x in (np.inf, -np.inf, 1e20, -1e20):
        c, t = R.dense(np.array([x], np.float32), R.FLOAT, *K.REF_RANGE)
        assert c.sum() == 0 and t["n_samples"] == 0 and t["n_skipped"] == 0 and t["min"] == float(np.float32(x)) == t["max"]
    c, t = R.dense(np.array([np.nan], np.float32), R.FLOAT, *K.REF_RANGE)
    assert c.sum() == 0 and t["n_skipped"] == 1 and t["min"] == math.inf and t["min_at"] == -1
    assert s["n_skipped"] == 1 and s["min"] == -math.inf and s["max"] == math.inf and s["min_at"] == 1 and s["max_at"] == 0
    assert counter[19650] == 1 and counter[19651] == 2 and counter[1] == 1 and counter[0] == 1      # (8651.4 -> 8651 too; 8651.6 and -11001.6 miss)
    assert counter.sum() == s["n_samples"] == 9
    # at scale 1 a negative int is binned one up: (int)(-3 + 0.5) = -2
    assert R.samples_of([-3, -1, 0, 3], 1.0).tolist() == [-2, 0, 0, 3]


def test_trap_negative_symbols_come_last():
    v = np.array([5, -1, 0, -32768, 32767, -1, 7], np.int16)
    sym, cnt, s = R.symbols(v, R.SHORT)
    assert sym.tolist() == [0, 5, 7, 32767, 0xFFFF8000, 0xFFFFFFFF] and cnt.tolist() == [1, 1, 1, 1, 1, 2]
    assert (s["n_symbols"], s["n_unique"], s["n_repeated"], s["max_count"]) == (6, 5, 1, 2)
    z = np.array([0.0, -0.0, np.nan, 1.0], np.float32)
    z2 = z.copy()
    z2.view(np.uint32)[2] = 0x7FC00001                                     # another NaN payload
    sym, cnt, s = R.symbols(np.concatenate([z, z2]), R.FLOAT)
    assert sym.tolist() == [0, 0x3F800000, 0x7FC00000, 0x7FC00001, 0x80000000] and cnt.tolist() == [2, 2, 1, 1, 2]


def test_trap_the_two_zeroes():
    a, b = K.zero_blocks()
    sa, sb = R.dense(a, R.FLOAT, *K.REF_RANGE)[1], R.dense(b, R.FLOAT, *K.REF_RANGE)[1]
    assert R.bits(sa["min"]) == R.bits(-0.0) and sa["min_at"] == 1
    assert R.bits(sb["min"]) == R.bits(0.0) and sb["min_at"] == 1
    assert R.bits(sa["min"]) != R.bits(sb["min"])
    sc = R.dense(b[2:], R.FLOAT, *K.REF_RANGE)[1]
    assert R.bits(sc["min"]) == R.bits(-0.0) and sc["min_at"] == 1 and sa["min_at"] != sb["min_at"] + 2


def test_plan_model():
    assert R.plan(-11000, 8650, 1.0) == dict(n_counter=19651, base=-11000, n_bins=19652, scale_used=1.0)
    assert R.plan(0, 99, 0.9)["scale_used"] == float(np.float32(0.9)) != 0.9
    assert R.plan(-2 ** 31, 2 ** 31 - 1, 1.0)["n_counter"] == 0            # the difference wraps to 0
    assert R.plan(-2 ** 31, 2 ** 31 - 2, 1.0) is None                      # ... to -1
    assert R.plan(0, 10, float("nan")) is None and R.plan(0, 10, 0.0) is None and R.plan(0, 10, -1.0) is None
    assert R.plan(0, 2 ** 31 - 2, 4.0)["n_counter"] == 2 ** 31 - 1         # the cast saturates


def test_entropy_model():
    assert R.entropy([1, 1, 1, 1], 4, True) == 2.0 and R.entropy([1, 1, 1, 1], 4, False) == 2.0
    assert R.entropy([8], 8, True) == 0.0 and R.entropy([], 0, False) == 0.0
    assert R.entropy([0, -5, 2, 0, 2], 4, True) == 1.0
