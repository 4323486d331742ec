"""CPU-only: gf_tile_record_decode_batch_dev and gf_codec_master_decode_batch_i32_dev reject what the host can check with
GF_ERR_ARG before the context or a device is looked at, accept an empty batch, and without a device fail as the other _dev
entry points do (there is no CPU path behind them)."""
import ctypes as C

import numpy as np

from gridfour_amd import _lib

STD = np.array([1, 2, 0, 3], np.int32)          # the standard codec list (include/gvrs_hip_codec.h)


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _buffers():
    # host memory standing in for device memory, and for a context: the argument checks must come before either is touched
    fake = C.create_string_buffer(8192)
    return dict(ctx=C.cast(fake, C.c_void_p), keep=fake, blob=np.zeros(256, np.uint8), off=np.array([0, 64, 128], np.uint64),
                lens=np.array([64, 64], np.uint32), idx=np.zeros(2, np.int32), val=np.zeros(2 * 16, np.int32), st=np.zeros(2, np.int32))


def _records(L, b, ctx="ctx", codecs=STD, n_codecs=4, elem=0, rows=4, cols=4, n=2, blob="blob", off="off", val="val", st="st"):
    g = lambda k: None if k is None else (b[k] if k == "ctx" else _p(b[k]))
    return L.gf_tile_record_decode_batch_dev(g(ctx), None, None if codecs is None else _p(codecs), n_codecs, elem, rows, cols, n,
                                             g(blob), b["blob"].size, g(off), 1, _p(b["idx"]), g(val), g(st))


def _master(L, b, ctx="ctx", codecs=STD, n_codecs=4, rows=4, cols=4, n=2, blob="blob", off="off", lens="lens", val="val", st="st"):
    g = lambda k: None if k is None else (b[k] if k == "ctx" else _p(b[k]))
    return L.gf_codec_master_decode_batch_i32_dev(g(ctx), None, None if codecs is None else _p(codecs), n_codecs, rows, cols, n,
                                                  g(blob), b["blob"].size, g(off), g(lens), g(val), g(st))


def test_argument_checks_come_before_the_device():
    L = _lib.lib()
    b = _buffers()
    nine = np.array([1, 9, 0, 3], np.int32)
    many = np.ones(256, np.int32)
    for call in (_records, _master):
        for null in ("ctx", "blob", "off", "val", "st"):
            assert call(L, b, **{null: None}) == _lib.ERR_ARG, (call.__name__, null)
        assert call(L, b, codecs=None) == _lib.ERR_ARG
        assert call(L, b, rows=0) == _lib.ERR_ARG
        assert call(L, b, cols=0) == _lib.ERR_ARG
        assert call(L, b, codecs=nine) == _lib.ERR_ARG
        assert call(L, b, codecs=many, n_codecs=256) == _lib.ERR_ARG
    assert _master(L, b, lens=None) == _lib.ERR_ARG
    assert _master(L, b, n_codecs=0) == _lib.ERR_ARG          # as gf_codec_master_decode_batch_i32
    assert _records(L, b, elem=2) == _lib.ERR_ARG
    assert _records(L, b, elem=-1) == _lib.ERR_ARG
    assert (b["st"] == 0).all() and (b["val"] == 0).all() and (b["idx"] == 0).all()


def test_empty_batch_is_ok_and_valid_arguments_need_a_device():
    L = _lib.lib()
    b = _buffers()
    assert _records(L, b, n=0) == _lib.OK
    assert _master(L, b, n=0) == _lib.OK
    assert _records(L, b, n=0, codecs=None, n_codecs=0) == _lib.OK      # a file without codecs
    if L.gf_device_count() > 0:
        return
    # no device: what another _dev entry point says to the same stand-in context
    want = L.gf_huffman_decode_batch_i32_dev(b["ctx"], None, 4, 4, 2, _p(b["blob"]), b["blob"].size, _p(b["off"]), 0, _p(b["lens"]),
                                             _p(b["val"]), _p(b["st"]))
    assert want < 0
    assert _records(L, b) == want
    assert _master(L, b) == want
