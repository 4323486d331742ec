"""CPU-only: gf_block_downsample_rect against the model's rule, and gf_block_downsample_elems[_dev] and
gf_block_read_downsampled_elems[_dev] rejecting what the host can check with GF_ERR_ARG / GF_ERR_UNSUPPORTED before the context or
a device is looked at (host memory stands in for both and stays untouched); an empty output rectangle is GF_OK; without a device
valid arguments fail as the other _dev entry points do."""
import ctypes as C

import numpy as np

import downsample_ref as R
from gridfour_amd import _lib
from gridfour_amd.codec import _ELEM_SPEC

PLAIN = ("dev", "host")
RECORD = ("read_dev", "read_host")


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _buffers():
    fake = C.create_string_buffer(8192)
    return dict(ctx=C.cast(fake, C.c_void_p), keep=fake, blk=np.zeros((2, 64), np.int32), out=np.zeros((2, 64), np.int32),
                blob=np.zeros(256, np.uint8), off=np.array([0, 64, 128], np.uint64), st=np.zeros(4, np.int32))


def _untouched(b):
    assert (b["blk"] == 0).all() and (b["out"] == 0).all() and (b["blob"] == 0).all() and (b["st"] == 0).all()
    assert b["off"].tolist() == [0, 64, 128]


def _call(L, b, form, ctx="ctx", elems=(("int", 0), ("float", 0)), n_elems=None, rect=(1, 2, 6, 8), factor=2, spec=True, has_rect=True,
          blocks=True, outs=True, block_ptrs=None, out_ptrs=None, grid=(12, 14, 4, 4), scale=1.0, codecs=(0, 1), blob="blob", off="off", st="st"):
    """one call of either family; elems: (type name or number, fill_i) per element"""
    types = {"int": 0, "short": 1, "float": 2, "icf": 3}
    specs = np.zeros(max(len(elems), 1), _ELEM_SPEC)
    for e, (t, fill) in enumerate(elems):
        specs[e]["type"], specs[e]["fill_i"], specs[e]["scale"] = types.get(t, t), fill, scale
    ne = len(elems) if n_elems is None else n_elems
    n_ptr = max(len(elems), 1)
    bp = [b["blk"][e % 2].ctypes.data for e in range(n_ptr)] if block_ptrs is None else block_ptrs
    op = [b["out"][e % 2].ctypes.data for e in range(n_ptr)] if out_ptrs is None else out_ptrs
    pb, po = (C.c_void_p * n_ptr)(*bp), (C.c_void_p * n_ptr)(*op)
    r = np.array(rect, np.int32)
    g = lambda k: None if k is None else (b[k] if k == "ctx" else _p(b[k]))
    a_ctx, a_spec, a_rect = g(ctx), (_p(specs) if spec else None), (_p(r) if has_rect else None)
    a_out = po if outs else None
    if form == "dev":
        return L.gf_block_downsample_elems_dev(a_ctx, None, a_spec, ne, a_rect, factor, pb if blocks else None, a_out)
    if form == "host":
        return L.gf_block_downsample_elems(a_ctx, a_spec, ne, a_rect, factor, pb if blocks else None, a_out)
    cod = np.array(codecs, np.int32)
    gr = np.array(grid, np.int32)
    if form == "read_dev":
        return L.gf_block_read_downsampled_elems_dev(a_ctx, None, _p(cod), cod.size, a_spec, ne, _p(gr), a_rect, factor, 2, g(blob), 128, g(off), 1,
                                                     a_out, g(st))
    return L.gf_block_read_downsampled_elems(a_ctx, _p(cod), cod.size, a_spec, ne, _p(gr), a_rect, factor, 2, g(blob), g(off), 1,
                                             a_out, g(st))


def test_rect_equals_the_model():
    L = _lib.lib()
    out = np.full(4, 99, np.int32)
    for f in (1, 2, 3, 4, 5, 8, 67, 46340):
        for block in ((0, 0, 10, 10), (0, 0, 11, 13), (1, 2, 10, 10), (3, 6, 3, 3), (4, 4, 4, 4), (1, 0, 2, 9), (5, 5, 1, 1), (7, 9, 300, 401),
                      (2 ** 31 - 10, 2 ** 31 - 70, 9, 69), (0, 0, 2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
            b = np.array(block, np.int32)
            assert L.gf_block_downsample_rect(_p(b), f, _p(out)) == _lib.OK
            assert tuple(int(x) for x in out) == R.out_rect(block, f), (f, block)
    for f in (2, 3):                                                     # every phase, and the strips of a whole
        for row0 in range(2 * f):
            b = np.array((row0, row0 + 1, 20, 23), np.int32)
            assert L.gf_block_downsample_rect(_p(b), f, _p(out)) == _lib.OK and tuple(int(x) for x in out) == R.out_rect(tuple(b), f)
    b = np.array((0, 0, 5, 5), np.int32)
    assert L.gf_block_downsample_rect(_p(b), 6, _p(out)) == _lib.OK and tuple(out[2:]) == (0, 0)


def test_rect_rejects():
    L = _lib.lib()
    out = np.full(4, 99, np.int32)
    good = np.array((0, 0, 4, 4), np.int32)
    assert L.gf_block_downsample_rect(None, 2, _p(out)) == _lib.ERR_ARG and L.gf_block_downsample_rect(_p(good), 2, None) == _lib.ERR_ARG
    for f in (0, -1, -2 ** 31):
        assert L.gf_block_downsample_rect(_p(good), f, _p(out)) == _lib.ERR_ARG
    for block in ((-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, -4, 4)):
        assert L.gf_block_downsample_rect(_p(np.array(block, np.int32)), 2, _p(out)) == _lib.ERR_ARG, block
    for f in (46341, 2 ** 31 - 1):
        assert L.gf_block_downsample_rect(_p(good), f, _p(out)) == _lib.ERR_UNSUPPORTED
        assert L.gf_block_downsample_rect(_p(np.array((0, 0, 0, 4), np.int32)), f, _p(out)) == _lib.ERR_ARG      # ARG comes first
    assert (out == 99).all()


def test_arguments_are_checked_before_the_device():
    L = _lib.lib()
    b = _buffers()
    for form in PLAIN + RECORD:
        bad = lambda **kw: _call(L, b, form, **kw) == _lib.ERR_ARG
        assert bad(ctx=None) and bad(spec=False) and bad(has_rect=False) and bad(outs=False), form
        assert bad(n_elems=0) and bad(n_elems=-1) and bad(n_elems=17), form
        for t in (-1, 4, 99):
            assert bad(elems=(("int", 0), (t, 0))), (form, t)
        for f in (0, -1, -2 ** 31):
            assert bad(factor=f), (form, f)
        for rect in ((-1, 2, 6, 8), (1, -2, 6, 8), (1, 2, 0, 8), (1, 2, 6, 0), (1, 2, -6, 8)):
            assert bad(rect=rect), (form, rect)
        assert bad(elems=(("short", 32768),)) and bad(elems=(("int", 0), ("short", -32769))), form
        ok_b, ok_o = b["blk"][0].ctypes.data, b["out"][0].ctypes.data
        assert bad(out_ptrs=[ok_o, 0]) and bad(out_ptrs=[ok_o + 2, ok_o]) and bad(out_ptrs=[ok_o, ok_o + 1]), form
        assert bad(factor=46341, rect=(1, 2, 0, 8)) and bad(factor=46341, n_elems=0), form          # ARG before UNSUPPORTED
    for form in PLAIN:
        bad = lambda **kw: _call(L, b, form, **kw) == _lib.ERR_ARG
        ok_b = b["blk"][0].ctypes.data
        assert bad(blocks=False) and bad(block_ptrs=[0, ok_b]) and bad(block_ptrs=[ok_b, ok_b + 2]) and bad(block_ptrs=[ok_b + 3, ok_b]), form
        assert bad(elems=(("icf", 0), ("short", 40000))), form                                      # ARG before UNSUPPORTED
    for form in RECORD:                                                                             # what the block read rejects
        bad = lambda **kw: _call(L, b, form, **kw) == _lib.ERR_ARG
        assert bad(blob=None) and bad(off=None) and bad(st=None), form
        assert bad(rect=(1, 2, 12, 8)) and bad(rect=(1, 2, 6, 13)), form                            # not inside the grid
        assert bad(grid=(12, 14, 0, 4)) and bad(grid=(0, 14, 4, 4)), form
        assert bad(elems=(("icf", 0),), scale=0.0) and bad(elems=(("icf", 0),), scale=float("nan")), form
        assert bad(codecs=(0, 9)), form
    _untouched(b)


def test_unsupported():
    L = _lib.lib()
    b = _buffers()
    for form in PLAIN + RECORD:
        for f in (46341, 2 ** 31 - 1):
            assert _call(L, b, form, factor=f) == _lib.ERR_UNSUPPORTED, (form, f)
    for form in PLAIN:                                                    # an int-coded float is averaged on its codes: read it as INT
        assert _call(L, b, form, elems=(("icf", 0),)) == _lib.ERR_UNSUPPORTED
        assert _call(L, b, form, elems=(("int", 0), ("icf", 0)), rect=(1, 2, 1, 1)) == _lib.ERR_UNSUPPORTED    # also with an empty result
    _untouched(b)


def test_an_empty_result_is_ok():
    L = _lib.lib()
    b = _buffers()
    for form in PLAIN:
        assert _call(L, b, form, rect=(1, 2, 2, 8), factor=3) == _lib.OK          # rows 1..2 hold no whole window of 3
        assert _call(L, b, form, rect=(1, 2, 6, 8), factor=46340) == _lib.OK
        assert _call(L, b, form, rect=(0, 0, 1, 1)) == _lib.OK
    _untouched(b)


def test_valid_arguments_need_a_device():
    """what passes the checks runs with a device; without one it fails as another _dev entry point does on the same stand-in
    context (there is no CPU path behind these calls)"""
    L = _lib.lib()
    if L.gf_device_count() > 0:
        return
    b = _buffers()
    lens = np.array([64, 64], np.uint32)
    val = np.zeros((2, 16), np.int32)
    want = L.gf_huffman_decode_batch_i32_dev(b["ctx"], None, 4, 4, 2, _p(b["blob"]), 256, _p(b["off"]), 0, _p(lens), _p(val), _p(b["st"]))
    assert want < 0
    for form in PLAIN + RECORD:
        assert _call(L, b, form) == want, form
        assert _call(L, b, form, elems=(("short", -32768),), factor=3) == want, form
    for form in RECORD:
        assert _call(L, b, form, elems=(("icf", 5), ("float", 0))) == want, form                       # ICF is taken as codes here
        assert _call(L, b, form, rect=(1, 2, 2, 8), factor=3) == want, form                            # an empty result still reads
        assert _call(L, b, form, factor=46340) == want, form
    _untouched(b)
