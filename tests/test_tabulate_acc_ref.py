"""CPU-only: the numpy model of merged symbol tables and accumulated strips (tests/tabulate_acc_ref.py) held to a literal
transcription of the reference's two loops (EntropyTabulator.java:227-297) run over strips with a dict for its file of counters, the
wrap cases on hand-built tables, n_samples past 2^32, the SHORT symbol order, and gf_tab_entropy_counts on an accumulated table."""
import numpy as np

import tabulate_acc_ref as A
import tabulate_cases as K
import tabulate_ref as R
from gridfour_amd import _lib
from test_tabulate_args import _entropy


def _cuts(n, k, rng):
    at = np.sort(rng.choice(np.arange(1, n), k - 1, replace=False)) if k > 1 else np.zeros(0, np.int64)
    return [0] + at.tolist() + [n]


def test_model_equals_the_reference_loops_over_strips():
    rng = np.random.default_rng(21)
    for elem_type in (R.INT, R.SHORT, R.FLOAT):
        v = K.dem_like(rng, 3000, elem_type, -300, 500)
        whole = R.symbols(v, elem_type)
        for k in (1, 2, 5, 37):
            c = _cuts(v.size, k, rng)
            strips = [v[a:b] for a, b in zip(c[:-1], c[1:])] + [v[:0]]       # and one empty strip
            lit, n_symbols_ref, _ = A.strips_literal(strips, elem_type)
            got = A.accumulate(strips, elem_type)
            assert A.same(got, lit) and n_symbols_ref == got[2]["n_symbols"], (elem_type, k)
            assert A.same(got, whole), (elem_type, k)                       # no wrap: the one-call table of tests/tabulate_ref.py


def test_counts_wrap_as_a_java_int_and_the_entry_stays():
    a = A.table([5, 9, 11], [2 ** 31 - 1, -1, 3])
    b = A.table([5, 9, 12], [1, 1, 1])
    sym, cnt, s = A.merge(a, b)
    assert sym.tolist() == [5, 9, 11, 12] and cnt.tolist() == [-2 ** 31, 0, 3, 1]
    assert (s["n_symbols"], s["n_unique"], s["n_repeated"], s["max_count"]) == (4, 1, 1, 3)
    # the reference's loop from a file that holds 2^31 - 1 and -1 for the two symbols: the same counters; its nSymbols counts the
    # symbol whose counter passes through 0 once more, ours counts distinct symbols (the stated deviation)
    lit, n_symbols_ref, file = A.strips_literal([np.array([5, 9, 9], np.int32)], R.INT, counts={5: 2 ** 31 - 1, 9: -1})
    assert file == {5: -2 ** 31, 9: 1} and n_symbols_ref == 1
    none = A.merge(A.table([7], [-2 ** 31]), A.table([7], [-2 ** 31]))
    assert none[1].tolist() == [0] and none[2]["max_count"] == 0 and none[2]["n_symbols"] == 1 and none[2]["n_unique"] == 0


def test_n_samples_is_an_int64_and_flags_are_sticky():
    a = A.table([1, 2], [5, 6], n_samples=2 ** 32 + 11)
    b = A.table([2, 3], [1, 1], n_samples=2 ** 33)
    s = A.merge(a, b)[2]
    assert s["n_samples"] == 2 ** 32 + 11 + 2 ** 33 and s["reserved"] == 0
    cut = A.table([1, 2], [5, 6], n_samples=40, n_symbols=9)              # it held 9 symbols once
    m = A.merge(cut, b)
    assert m[2]["reserved"] == A.TRUNCATED and m[0].tolist() == [1, 2, 3]
    assert A.merge(m, a)[2]["reserved"] == A.TRUNCATED and A.merge(a, m)[2]["reserved"] == A.TRUNCATED
    assert A.merge(a, b, cap_a=1)[2]["reserved"] == A.TRUNCATED and A.merge(a, b, cap_a=1)[0].tolist() == [1, 2, 3]
    assert A.cut(m, 2)[2]["n_written"] == 2 and A.cut(m, 2)[2]["n_symbols"] == 3


def test_short_symbols_in_table_order():
    v = np.array([-1, 0, 32767, -32768, 5, -2], np.int16)
    assert A.short_order(v).tolist() == [0, 5, 32767, 0xFFFF8000, 0xFFFFFFFE, 0xFFFFFFFF]
    assert np.array_equal(A.short_order(v), R.symbols(v, R.SHORT)[0])
    every = np.arange(-32768, 32768).astype(np.int16)
    order = A.short_order(every)
    assert order.size == 65536 and np.array_equal(order & np.uint32(0xFFFF), np.arange(65536, dtype=np.uint32))


def test_entropy_of_an_accumulated_table():
    L = _lib.lib()
    rng = np.random.default_rng(22)
    v = K.dem_like(rng, 20000, R.SHORT)
    t = A.accumulate([v[:7000], v[7000:7001], v[7001:]], R.SHORT)
    whole = R.symbols(v, R.SHORT)
    for kahan in (1, 0):
        got = _entropy(L, t[1], t[2]["n_samples"], kahan)
        assert R.bits(got) == R.bits(R.entropy(whole[1], v.size, bool(kahan))) and 0.0 < got < 16.0
    wrapped = A.merge(A.table([1, 2, 3], [2 ** 31 - 1, 4, -1]), A.table([1, 3], [1, 1]))       # counts <= 0 are skipped
    assert wrapped[1].tolist() == [-2 ** 31, 4, 0]
    assert R.bits(_entropy(L, wrapped[1], 4, 1)) == R.bits(R.entropy(wrapped[1], 4, True)) == R.bits(R.entropy([4], 4, True))
