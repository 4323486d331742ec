"""CPU-only: gf_canon_analyze_batch rejects bad arguments with GF_ERR_ARG before it touches the context or a device
(as gf_huffman_analyze_batch does: null pointers, offsets that do not ascend or span more than 4 GB per packing)."""
import ctypes as C

import numpy as np

import gridfour_amd
from gridfour_amd import _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_canon_analyze_batch_argument_checks():
    L = _lib.lib()
    stats = np.zeros(6, dtype=gridfour_amd.CANON_STATS_DTYPE)
    esc = np.zeros(6, np.int64)
    status = np.zeros(2, np.int32)
    blob = np.zeros(64, np.uint8)
    good = np.array([0, 10, 20], np.uint64)
    # a stand-in for a context: the checks must fail before it is looked at
    fake = C.create_string_buffer(4096)
    ctx = C.cast(fake, C.c_void_p)
    assert stats.itemsize == 72
    assert L.gf_canon_analyze_batch(None, 4, 4, 2, _p(blob), _p(good), _p(stats), _p(esc), _p(status)) == _lib.ERR_ARG
    assert L.gf_canon_analyze_batch(ctx, 4, 4, 2, _p(blob), _p(good), None, _p(esc), _p(status)) == _lib.ERR_ARG
    assert L.gf_canon_analyze_batch(ctx, 4, 4, 2, _p(blob), _p(good), _p(stats), None, _p(status)) == _lib.ERR_ARG
    assert L.gf_canon_analyze_batch(ctx, 4, 4, 2, None, _p(good), _p(stats), _p(esc), _p(status)) == _lib.ERR_ARG
    assert L.gf_canon_analyze_batch(ctx, 4, 4, 2, _p(blob), None, _p(stats), _p(esc), _p(status)) == _lib.ERR_ARG
    assert L.gf_canon_analyze_batch(ctx, 0, 4, 2, _p(blob), _p(good), _p(stats), _p(esc), _p(status)) == _lib.ERR_ARG
    for bad in ([0, 10, 5], [0, 2 ** 33, 2 ** 33 + 1]):
        offs = np.array(bad, np.uint64)
        assert L.gf_canon_analyze_batch(ctx, 4, 4, 2, _p(blob), _p(offs), _p(stats), _p(esc), _p(status)) == _lib.ERR_ARG
    assert (stats["n_tiles"] == 0).all() and (esc == 0).all()
