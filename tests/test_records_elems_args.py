"""CPU-only: gf_tile_record_decode_batch_elems_dev and gf_tile_record_decode_batch_elems reject what the host can check with
GF_ERR_ARG / GF_ERR_UNSUPPORTED before the context or a device is looked at, accept an empty batch, and without a device fail as
the other _dev entry points do (there is no CPU path behind them)."""
import ctypes as C

import numpy as np

from gridfour_amd import _lib
from gridfour_amd.codec import _ELEM_SPEC

STD = np.array([1, 2, 0, 3], np.int32)          # the standard codec list (include/gvrs_hip_codec.h)
INT, SHORT, FLOAT, ICF = 0, 1, 2, 3


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _specs(*types, scale=1.0):
    s = np.zeros(len(types), _ELEM_SPEC)
    s["type"] = types
    s["scale"] = scale
    return s


def _buffers():
    # host memory standing in for device memory, and for a context: the argument checks must come before either is touched
    fake = C.create_string_buffer(8192)
    return dict(ctx=C.cast(fake, C.c_void_p), keep=fake, blob=np.zeros(256, np.uint8), off=np.array([0, 64, 128], np.uint64),
                idx=np.zeros(2, np.int32), val=np.zeros((16, 2 * 16), np.int32), st=np.zeros(16 * 2, np.int32))


def _call(L, b, dev, ctx="ctx", codecs=STD, n_codecs=4, specs=None, n_elems=None, rows=4, cols=4, n=2, blob="blob", off="off",
          values="val", null_value=None, st="st", blob_shift=0):
    g = lambda k: None if k is None else (b[k] if k == "ctx" else _p(b[k]))
    specs = _specs(INT, FLOAT) if specs is None else specs
    n_elems = len(specs) if n_elems is None and specs is not False else n_elems
    ptrs = (C.c_void_p * 17)(*[b["val"][e % 16].ctypes.data for e in range(17)])
    if null_value is not None:
        ptrs[null_value] = None
    pv = None if values is None else ptrs
    ps = None if specs is False else _p(specs)
    pb = g(blob)
    if pb is not None and blob_shift:
        pb = C.c_void_p(pb.value + blob_shift)
    if dev:
        return L.gf_tile_record_decode_batch_elems_dev(g(ctx), None, None if codecs is None else _p(codecs), n_codecs, ps, n_elems, rows,
                                                       cols, n, pb, b["blob"].size, g(off), 1, _p(b["idx"]), pv, g(st))
    return L.gf_tile_record_decode_batch_elems(g(ctx), None if codecs is None else _p(codecs), n_codecs, ps, n_elems, rows, cols, n, pb,
                                               g(off), 1, _p(b["idx"]), pv, g(st))


def test_argument_checks_come_before_the_device():
    L = _lib.lib()
    b = _buffers()
    nine = np.array([1, 9, 0, 3], np.int32)
    many = np.ones(256, np.int32)
    for dev in (True, False):
        for null in ("ctx", "blob", "off", "st"):
            assert _call(L, b, dev, **{null: None}) == _lib.ERR_ARG, (dev, null)
        assert _call(L, b, dev, values=None) == _lib.ERR_ARG
        assert _call(L, b, dev, null_value=1) == _lib.ERR_ARG                          # one of the n_elems value pointers
        assert _call(L, b, dev, specs=False, n_elems=2) == _lib.ERR_ARG                # elems == NULL
        assert _call(L, b, dev, codecs=None) == _lib.ERR_ARG
        assert _call(L, b, dev, n_elems=0) == _lib.ERR_ARG
        assert _call(L, b, dev, n_elems=-1) == _lib.ERR_ARG
        assert _call(L, b, dev, specs=_specs(*([INT] * 17))) == _lib.ERR_ARG           # > GF_MAX_ELEMS
        assert _call(L, b, dev, specs=_specs(INT, 4)) == _lib.ERR_ARG
        assert _call(L, b, dev, specs=_specs(-1)) == _lib.ERR_ARG
        assert _call(L, b, dev, specs=_specs(INT, ICF, scale=0.0)) == _lib.ERR_ARG
        assert _call(L, b, dev, specs=_specs(ICF, scale=-0.0)) == _lib.ERR_ARG
        assert _call(L, b, dev, specs=_specs(ICF, FLOAT, scale=np.nan)) == _lib.ERR_ARG
        assert _call(L, b, dev, codecs=nine) == _lib.ERR_ARG
        assert _call(L, b, dev, codecs=many, n_codecs=256) == _lib.ERR_ARG
        assert _call(L, b, dev, rows=0) == _lib.ERR_ARG
        assert _call(L, b, dev, cols=0) == _lib.ERR_ARG
    for shift in (1, 2, 3):
        assert _call(L, b, True, blob_shift=shift) == _lib.ERR_ARG                     # an unaligned d_blob
    assert (b["st"] == 0).all() and (b["val"] == 0).all() and (b["idx"] == 0).all()


def test_instance_count_limit_is_unsupported():
    """n_elems * n_tiles > 0x7fffffff: instance numbers travel as 32 bits.  Nothing is read: the offsets array has three entries."""
    L = _lib.lib()
    b = _buffers()
    for dev in (True, False):
        assert _call(L, b, dev, specs=_specs(INT), n=2**31) == _lib.ERR_UNSUPPORTED
        assert _call(L, b, dev, specs=_specs(INT, FLOAT), n=2**30) == _lib.ERR_UNSUPPORTED
        assert _call(L, b, dev, specs=_specs(*([SHORT] * 16)), n=2**27) == _lib.ERR_UNSUPPORTED
        assert _call(L, b, dev, specs=_specs(INT), n=2**40) == _lib.ERR_UNSUPPORTED
        assert _call(L, b, dev, specs=_specs(INT, 7), n=2**31) == _lib.ERR_ARG           # the argument checks come first
    assert (b["st"] == 0).all() and (b["val"] == 0).all()


def test_empty_batch_is_ok_and_valid_arguments_need_a_device():
    L = _lib.lib()
    b = _buffers()
    for dev in (True, False):
        assert _call(L, b, dev, n=0) == _lib.OK
        assert _call(L, b, dev, n=0, codecs=None, n_codecs=0) == _lib.OK              # a file without codecs
        assert _call(L, b, dev, n=0, specs=_specs(*([ICF] * 16))) == _lib.OK
    if L.gf_device_count() > 0:
        return
    # no device: what another _dev entry point says to the same stand-in context
    lens = np.array([64, 64], np.uint32)
    want = L.gf_huffman_decode_batch_i32_dev(b["ctx"], None, 4, 4, 2, _p(b["blob"]), b["blob"].size, _p(b["off"]), 0, _p(lens),
                                             _p(b["val"]), _p(b["st"]))
    assert want < 0
    for dev in (True, False):
        assert _call(L, b, dev) == want
