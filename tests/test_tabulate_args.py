"""CPU-only: gf_block_tabulate_dense[_dev] and gf_block_tabulate_symbols[_dev] rejecting what the host can check with GF_ERR_ARG /
GF_ERR_UNSUPPORTED before the context or a device is looked at (host memory stands in for both and stays untouched),
gf_tab_dense_plan_of against the model's plan, and gf_tab_entropy_counts against the model's two sums bit for bit (both sides use
the C library's log, so equality is the condition); without a device valid arguments fail as the other _dev entry points do."""
import ctypes as C

import numpy as np
import pytest

import tabulate_cases as K
import tabulate_ref as R
from gridfour_amd import _lib
from gridfour_amd.codec import _TAB_DENSE, _TAB_DENSE_PLAN, TAB_ACCUMULATE, TAB_SKIP_FILL, TAB_SUMMARY, TAB_SYMBOLS

DENSE = ("dense_dev", "dense_host")
SYMBOLS = ("symbols_dev", "symbols_host")
TYPES = {"int": 0, "short": 1, "float": 2, "icf": 3}


def _p(a, off=0):
    return C.c_void_p(a.ctypes.data + off)


def _buffers():
    fake = C.create_string_buffer(8192)
    return dict(ctx=C.cast(fake, C.c_void_p), keep=fake, blk=np.zeros(64, np.int32), counter=np.zeros(64, np.int32), summary=np.zeros(16, np.int64),
                symbols=np.zeros(64, np.uint32), counts=np.zeros(64, np.int32))


def _untouched(b):
    assert bytes(b["keep"].raw) == bytes(8192)
    assert all((b[k] == 0).all() for k in ("blk", "counter", "summary", "symbols", "counts"))


def _call(L, b, form, ctx="ctx", elem="int", fill_i=0, flags=0, blk="blk", blk_off=0, n_cells=16, first_cell=0, spec=(0, 9, 1.0), counter="counter",
          counter_off=0, summary="summary", summary_off=0, symbols="symbols", counts="counts", cap=8):
    g = lambda k, off=0: None if k is None else (b[k] if k == "ctx" else _p(b[k], off))
    et = TYPES.get(elem, elem)
    if form in DENSE:
        sp = None
        if spec is not None:
            sp = np.zeros(1, _TAB_DENSE)
            sp["def_min"], sp["def_max"], sp["scale"] = spec
        a_spec = None if sp is None else _p(sp)
        if form == "dense_dev":
            return L.gf_block_tabulate_dense_dev(g(ctx), None, et, fill_i, flags, g(blk, blk_off), n_cells, first_cell, a_spec,
                                                 g(counter, counter_off), g(summary, summary_off))
        return L.gf_block_tabulate_dense(g(ctx), et, fill_i, flags, g(blk, blk_off), n_cells, first_cell, a_spec, g(counter, counter_off),
                                         g(summary, summary_off))
    if form == "symbols_dev":
        return L.gf_block_tabulate_symbols_dev(g(ctx), None, et, g(blk, blk_off), n_cells, g(symbols), g(counts), cap, g(summary, summary_off))
    return L.gf_block_tabulate_symbols(g(ctx), et, g(blk, blk_off), n_cells, g(symbols), g(counts), cap, g(summary, summary_off))


def test_arguments_are_checked_before_the_device():
    L = _lib.lib()
    b = _buffers()
    for form in DENSE + SYMBOLS:
        bad = lambda **kw: _call(L, b, form, **kw) == _lib.ERR_ARG
        assert bad(ctx=None) and bad(blk=None) and bad(summary=None), form
        for t in (-1, 4, 99):
            assert bad(elem=t), (form, t)
        assert bad(n_cells=-1) and bad(n_cells=-2 ** 63), form
        assert bad(blk_off=1) and bad(blk_off=2) and bad(blk_off=3) and not bad(blk_off=4), form
        assert bad(summary_off=4) and bad(summary_off=1) and not bad(summary_off=8), form
        assert bad(elem="icf", n_cells=-1) and bad(elem="icf", summary_off=4), form                # ARG before UNSUPPORTED
    for form in DENSE:
        bad = lambda **kw: _call(L, b, form, **kw) == _lib.ERR_ARG
        assert bad(spec=None) and bad(counter=None) and bad(counter_off=2), form
        assert bad(first_cell=-1), form
        assert bad(elem="short", fill_i=32768) and bad(elem="short", fill_i=-32769) and not bad(elem="short", fill_i=-32768), form
        assert not bad(elem="int", fill_i=-2 ** 31), form
        for flags in (4, 8, -1, TAB_ACCUMULATE | TAB_SKIP_FILL | 16):
            assert bad(flags=flags), (form, flags)
        for spec in ((0, 9, 0.0), (0, 9, -1.0), (0, 9, float("nan")), (0, 9, -float("inf")), (5, 3, 1.0), (-2 ** 31, 2 ** 31 - 2, 1.0), (0, -2, 1.0)):
            assert bad(spec=spec), (form, spec)
        assert bad(elem="icf", spec=(0, 9, 0.0)) and bad(spec=(0, 2 ** 30, 1.0), flags=4), form    # ARG before UNSUPPORTED
    for form in SYMBOLS:
        bad = lambda **kw: _call(L, b, form, **kw) == _lib.ERR_ARG
        assert bad(symbols=None) and bad(counts=None) and bad(symbols=None, counts=None), form
        assert bad(elem="icf", symbols=None), form
    _untouched(b)


def test_unsupported():
    L = _lib.lib()
    b = _buffers()
    for form in DENSE + SYMBOLS:
        assert _call(L, b, form, elem="icf") == _lib.ERR_UNSUPPORTED, form
        assert _call(L, b, form, elem="icf", n_cells=0) == _lib.ERR_UNSUPPORTED, form
    for form in DENSE:
        assert _call(L, b, form, spec=(0, 2 ** 28 - 1, 1.0)) == _lib.ERR_UNSUPPORTED, form          # n_bins = 2^28 + 1
        assert _call(L, b, form, spec=(0, 2 ** 31 - 2, 4.0)) == _lib.ERR_UNSUPPORTED, form          # the saturated count
        assert _call(L, b, form, n_cells=2 ** 40 + 1) == _lib.ERR_UNSUPPORTED, form                 # one call's cells
    for form in SYMBOLS:
        assert _call(L, b, form, n_cells=2 ** 31) == _lib.ERR_UNSUPPORTED, form
        assert _call(L, b, form, n_cells=2 ** 40, cap=0, symbols=None, counts=None) == _lib.ERR_UNSUPPORTED, form
    _untouched(b)


def test_valid_arguments_need_a_device():
    """what passes the checks runs with a device; without one it fails as another _dev entry point does on the same stand-in context
    (there is no CPU path behind these calls)"""
    L = _lib.lib()
    if L.gf_device_count() > 0:
        return
    b = _buffers()
    blob, off, lens = np.zeros(256, np.uint8), np.array([0, 64, 128], np.uint64), np.array([64, 64], np.uint32)
    val, st = np.zeros((2, 16), np.int32), np.zeros(4, np.int32)
    want = L.gf_huffman_decode_batch_i32_dev(b["ctx"], None, 4, 4, 2, _p(blob), 256, _p(off), 0, _p(lens), _p(val), _p(st))
    assert want < 0
    for form in DENSE + SYMBOLS:
        for elem in ("int", "short", "float"):
            assert _call(L, b, form, elem=elem) == want, (form, elem)
        assert _call(L, b, form, n_cells=0) == want, form
    for form in DENSE:
        assert _call(L, b, form, flags=TAB_ACCUMULATE | TAB_SKIP_FILL, spec=(0, 2 ** 28 - 2, 1.0), first_cell=2 ** 40) == want, form      # n_bins = 2^28
    for form in SYMBOLS:
        assert _call(L, b, form, cap=0, symbols=None, counts=None) == want, form
        assert _call(L, b, form, n_cells=2 ** 31 - 1) == want, form
    _untouched(b)


PLANS = [K.REF_RANGE, (0, 99, 0.9), (-50, 60, 0.7), (10, 300, 0.35), (-2 ** 31, 2 ** 31 - 1, 1.0), (-7, -7, 1.0), (0, -1, 1.0), (-1000, 1000, 1e-3),
         (-2 ** 31, -2 ** 31 + 2 ** 28 - 2, 1.0), (2 ** 31 - 100, 2 ** 31 - 1, 1.0), (0, 2 ** 28 - 3, 1.0), (0, 2 ** 28 - 2, 1.0), (1, 2 ** 27 - 1, 2.0),
         (0, 19651, 0.9), (3, 9, 1e-300)]


def test_plan_equals_the_model():
    L = _lib.lib()
    sp, out = np.zeros(1, _TAB_DENSE), np.zeros(1, _TAB_DENSE_PLAN)
    for def_min, def_max, scale in PLANS:
        sp["def_min"], sp["def_max"], sp["scale"] = def_min, def_max, scale
        out[:] = 0
        assert L.gf_tab_dense_plan_of(_p(sp), _p(out)) == _lib.OK, (def_min, def_max, scale)
        assert {k: out[k][0].item() for k in out.dtype.names} == R.plan(def_min, def_max, scale), (def_min, def_max, scale)
    assert R.plan(*K.REF_RANGE)["n_counter"] == 19651 and R.plan(*K.REF_RANGE)["base"] == -11000
    assert R.plan(-2 ** 31, 2 ** 31 - 1, 1.0)["n_bins"] == 1                                       # the wrapped difference
    assert R.plan(0, 2 ** 28 - 2, 1.0)["n_bins"] == 2 ** 28                                        # the cap itself
    out[:] = 0
    for spec, want in (((0, 2 ** 28 - 1, 1.0), _lib.ERR_UNSUPPORTED), ((0, 2 ** 31 - 2, 4.0), _lib.ERR_UNSUPPORTED), ((5, 3, 1.0), _lib.ERR_ARG),
                       ((-2 ** 31, 2 ** 31 - 2, 1.0), _lib.ERR_ARG), ((0, 9, 0.0), _lib.ERR_ARG), ((0, 9, float("nan")), _lib.ERR_ARG),
                       ((0, 9, -2.0), _lib.ERR_ARG)):
        sp["def_min"], sp["def_max"], sp["scale"] = spec
        assert L.gf_tab_dense_plan_of(_p(sp), _p(out)) == want, spec
        assert (R.plan(*spec) is None) == (want == _lib.ERR_ARG)
    assert L.gf_tab_dense_plan_of(None, _p(out)) == _lib.ERR_ARG and L.gf_tab_dense_plan_of(_p(sp), None) == _lib.ERR_ARG
    assert bytes(out.tobytes()) == bytes(out.nbytes)


def _entropy(L, counts, n_samples, kahan):
    counts, e = np.ascontiguousarray(counts, np.int32), C.c_double(-1.0)
    assert L.gf_tab_entropy_counts(_p(counts) if counts.size else None, counts.size, n_samples, kahan, C.byref(e)) == _lib.OK
    return e.value


def test_entropy_equals_the_model_bit_for_bit():
    L = _lib.lib()
    rng = np.random.default_rng(9)
    big = np.exp(rng.uniform(0.0, np.log(1e6), 12000)).astype(np.int32)    # 1 .. 10^6, every magnitude
    big[:3] = (1, 10 ** 6, 999999)
    mixed = big.copy()
    mixed[1::7], mixed[4::11] = 0, -rng.integers(1, 1000, mixed[4::11].size)
    for counts in (big, mixed, big[:1], np.array([1, 1, 1, 1], np.int32), np.array([0, -3], np.int32), np.zeros(0, np.int32)):
        n = int(counts[counts > 0].sum(dtype=np.int64))
        for kahan in (1, 0):
            if n == 0 and kahan:
                continue
            got, want = _entropy(L, counts, n, kahan), R.entropy(counts, n, bool(kahan))
            assert R.bits(got) == R.bits(want), (counts.size, kahan, got, want)
    assert _entropy(L, big, 0, 0) == 0.0                                   # getEntropy's early return
    a, b = _entropy(L, big, int(big.sum(dtype=np.int64)), 1), _entropy(L, big, int(big.sum(dtype=np.int64)), 0)
    assert 0.0 < a < 32.0 and abs(a - b) < 1e-9
    n_big, back = int(big.sum(dtype=np.int64)), np.ascontiguousarray(big[::-1])
    for kahan in (1, 0):                                                   # "in the order given": the reversed table against the model on it
        assert R.bits(_entropy(L, back, n_big, kahan)) == R.bits(R.entropy(back, n_big, bool(kahan)))
    assert R.bits(R.entropy(back, n_big, False)) != R.bits(R.entropy(big, n_big, False))      # ... and the plain sum does depend on the order
    e = C.c_double()
    assert L.gf_tab_entropy_counts(None, 3, 3, 1, C.byref(e)) == _lib.ERR_ARG and L.gf_tab_entropy_counts(_p(big), 3, 3, 1, None) == _lib.ERR_ARG
    assert L.gf_tab_entropy_counts(_p(big), 3, -1, 1, C.byref(e)) == _lib.ERR_ARG and L.gf_tab_entropy_counts(_p(big), 3, 3, 2, C.byref(e)) == _lib.ERR_ARG


def test_struct_sizes():
    assert _TAB_DENSE.itemsize == 16 and _TAB_DENSE_PLAN.itemsize == 24 and TAB_SUMMARY.itemsize == 72 and TAB_SYMBOLS.itemsize == 48
