"""CPU-only: gf_tab_symbols_merge[_dev] and gf_block_tabulate_symbols_acc[_dev] rejecting what the host can check, in the order the
header states -- NULLs, element type and cell count, misaligned blocks and tables, caps without arrays, outputs that overlap inputs:
GF_ERR_ARG; then GF_ELEM_ICF, n_cells past 2^31 - 1 and caps past 2^31 - 1: GF_ERR_UNSUPPORTED -- before the context or a device is
looked at (host memory stands in for both and stays untouched); without a device valid arguments fail as another entry point does."""
import ctypes as C

import numpy as np

from gridfour_amd import _lib
from gridfour_amd.codec import TAB_SYMBOLS

MERGE = ("merge_dev", "merge_host")
ACC = ("acc_dev", "acc_host")
TYPES = {"int": 0, "short": 1, "float": 2, "icf": 3}
TABLES = ("sym_a", "cnt_a", "sym_b", "cnt_b", "sym_out", "cnt_out")


def _p(a, off=0):
    return C.c_void_p(a.ctypes.data + off)


def _buffers(last="a"):
    """every array a view of one arena, the outputs in front and the tables of `last` at its end: a cap of 2^31 entries on them
    reaches far behind the arena and still overlaps no output"""
    fake = C.create_string_buffer(8192)
    arena = np.zeros(16 * 64, np.uint32)
    order = ["sum_out", "sym_out", "cnt_out", "blk", "sum_a", "sum_b"] + [k + "_" + t for t in ("b" if last == "a" else "a", last) for k in ("sym", "cnt")]
    b = dict(ctx=C.cast(fake, C.c_void_p), keep=fake, arena=arena)
    for i, k in enumerate(order):
        b[k] = arena[64 * i:64 * (i + 1)].view(np.int64 if k.startswith("sum") else np.int32 if k == "blk" else np.uint32)
    return b


def _untouched(b):
    assert bytes(b["keep"].raw) == bytes(8192)
    assert all((b[k] == 0).all() for k in b if k not in ("ctx", "keep"))


def _call(L, b, form, ctx="ctx", elem="int", blk="blk", n_cells=16, cap_a=8, cap_b=8, cap_out=16, off=None, **names):
    """names: which buffer stands for an argument (None: NULL), e.g. sym_out="sym_a" for an overlap; off: {argument: byte offset}"""
    off = off or {}

    def g(arg):
        k = names.get(arg, arg)
        return None if k is None else (b[k] if k == "ctx" else _p(b[k], off.get(arg, 0)))
    et = TYPES.get(elem, elem)
    c = None if ctx is None else b["ctx"]
    if form in MERGE:
        fn = L.gf_tab_symbols_merge_dev if form == "merge_dev" else L.gf_tab_symbols_merge
        return fn(c, g("sym_a"), g("cnt_a"), g("sum_a"), cap_a, g("sym_b"), g("cnt_b"), g("sum_b"), cap_b, g("sym_out"), g("cnt_out"), cap_out,
                  g("sum_out"))
    fn = L.gf_block_tabulate_symbols_acc_dev if form == "acc_dev" else L.gf_block_tabulate_symbols_acc
    blk_p = None if blk is None else _p(b[blk], off.get("blk", 0))
    return fn(c, et, blk_p, n_cells, g("sym_a"), g("cnt_a"), g("sum_a"), cap_a, g("sym_out"), g("cnt_out"), cap_out, g("sum_out"))


def test_arguments_are_checked_before_the_device():
    L = _lib.lib()
    b = _buffers()
    for form in MERGE + ACC:
        bad = lambda **kw: _call(L, b, form, **kw) == _lib.ERR_ARG
        assert bad(ctx=None) and bad(sum_out=None), form
        assert bad(sym_out=None) and bad(cnt_out=None) and not bad(sym_out=None, cnt_out=None, cap_out=0), form          # caps without arrays
        for arg in ("sym_a", "cnt_a", "sym_out", "cnt_out"):                                                             # misaligned tables
            assert bad(off={arg: 1}) and bad(off={arg: 2}) and not bad(off={arg: 4}), (form, arg)
        assert bad(off={"sum_a": 4}) and bad(off={"sum_out": 4}) and not bad(off={"sum_out": 8}), form
        for out, into in (("sym_out", "sym_a"), ("sym_out", "cnt_a"), ("cnt_out", "sym_a"), ("cnt_out", "cnt_a"), ("sum_out", "sum_a"),
                          ("cnt_out", "sym_out")):                                                                        # overlapping in and out
            assert bad(**{out: into}), (form, out, into)
        assert bad(sym_out="sym_a", off={"sym_out": 28}) and not bad(sym_out="sym_a", off={"sym_out": 32}), form          # the last entry; behind it
        assert bad(sym_out="sum_a") and bad(sum_out="sym_a"), form
    for form in MERGE:
        bad = lambda **kw: _call(L, b, form, **kw) == _lib.ERR_ARG
        assert bad(sum_a=None) and bad(sum_b=None), form
        assert bad(sym_a=None) and bad(cnt_b=None) and not bad(sym_a=None, cnt_a=None, cap_a=0), form
        assert bad(off={"sym_b": 2}) and bad(off={"sum_b": 4}) and bad(sym_out="cnt_b"), form
        assert bad(cap_a=2 ** 31, sum_out=None) and bad(cap_a=2 ** 31, sym_out="cnt_a"), form                             # ARG before UNSUPPORTED
    for form in ACC:
        bad = lambda **kw: _call(L, b, form, **kw) == _lib.ERR_ARG
        assert bad(blk=None) and bad(n_cells=-1) and bad(n_cells=-2 ** 63), form
        for t in (-1, 4, 99):
            assert bad(elem=t), (form, t)
        assert bad(off={"blk": 1}) and bad(off={"blk": 2}) and bad(off={"blk": 3}) and not bad(off={"blk": 4}), form
        assert bad(elem="short", off={"blk": 1}) and not bad(elem="short", off={"blk": 2}), form                          # a SHORT block: 2-byte aligned
        assert bad(sym_a=None) and bad(cnt_a=None), form                                                                  # one array of the in-table
        assert not bad(sym_a=None, cnt_a=None) and not bad(sum_a=None) and not bad(cap_a=0), form                         # ... an empty in-table
        assert bad(elem="icf", n_cells=-1) and bad(elem="icf", sum_out=None) and bad(n_cells=2 ** 31, sym_out="sym_a"), form   # ARG before UNSUPPORTED
    _untouched(b)


def test_unsupported():
    L = _lib.lib()
    b = _buffers()
    for form in MERGE:
        assert _call(L, b, form, cap_a=2 ** 31) == _lib.ERR_UNSUPPORTED and _call(L, _buffers("b"), form, cap_b=2 ** 31) == _lib.ERR_UNSUPPORTED, form
    for form in ACC:
        assert _call(L, b, form, elem="icf") == _lib.ERR_UNSUPPORTED and _call(L, b, form, elem="icf", n_cells=0) == _lib.ERR_UNSUPPORTED, form
        assert _call(L, b, form, n_cells=2 ** 31) == _lib.ERR_UNSUPPORTED and _call(L, b, form, n_cells=2 ** 40, cap_out=0, sym_out=None,
                                                                                     cnt_out=None) == _lib.ERR_UNSUPPORTED, form
        assert _call(L, b, form, cap_a=2 ** 31) == _lib.ERR_UNSUPPORTED, form
    _untouched(b)


def test_valid_arguments_need_a_device():
    """what passes the checks runs with a device; without one it fails as another _dev entry point does on the same stand-in context"""
    L = _lib.lib()
    if L.gf_device_count() > 0:
        return
    b = _buffers()
    blob, off, lens = np.zeros(256, np.uint8), np.array([0, 64, 128], np.uint64), np.array([64, 64], np.uint32)
    val, st = np.zeros((2, 16), np.int32), np.zeros(4, np.int32)
    want = L.gf_huffman_decode_batch_i32_dev(b["ctx"], None, 4, 4, 2, _p(blob), 256, _p(off), 0, _p(lens), _p(val), _p(st))
    assert want < 0
    for form in MERGE + ACC:
        assert _call(L, b, form) == want, form
        assert _call(L, b, form, cap_out=0, sym_out=None, cnt_out=None) == want, form
    for form in ACC:
        for elem in ("int", "short", "float"):
            assert _call(L, b, form, elem=elem, n_cells=2 ** 31 - 1 if form == "acc_dev" else 16) == want, (form, elem)
        assert _call(L, b, form, n_cells=0, sym_a=None, cnt_a=None, sum_a=None, cap_a=0) == want, form
    _untouched(b)


def test_struct_and_flag():
    from gridfour_amd.codec import TAB_SYM_INPUT_TRUNCATED
    assert TAB_SYMBOLS.itemsize == 48 and TAB_SYM_INPUT_TRUNCATED == 1
