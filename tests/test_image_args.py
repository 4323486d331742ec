"""CPU-only: the argument catalogue of the gf_image_* calls.  Every refusal comes back as its code before the context or a device
is looked at (host memory stands in for both and stays untouched), n_pixels == 0 and an empty reduced image are GF_OK, and without
a device valid arguments fail as another _dev entry point does on the same stand-in context."""
import ctypes as C

import numpy as np

import image_ref as M
from gridfour_amd import _lib

PLANE = ("split_dev", "join_dev", "split", "join")
REDUCE = ("reduce_dev", "reduce")
RECORD = ("write_dev", "read_dev", "write", "read")
ARG, UNSUPPORTED, OK = _lib.ERR_ARG, _lib.ERR_UNSUPPORTED, _lib.OK


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _buffers():
    fake = C.create_string_buffer(8192)
    return dict(ctx=C.cast(fake, C.c_void_p), keep=fake, argb=np.zeros(64, np.int32), planes=np.zeros((3, 64), np.int32),
                out=np.zeros(64, np.int32), blob=np.zeros(256, np.uint64), off=np.array([0, 64, 128], np.uint64), st=np.zeros(16, np.int32),
                idx=np.zeros(16, np.int32), used=np.zeros(64, np.uint8), new_off=np.zeros(16, np.uint64))


def _untouched(b):
    for k in ("argb", "planes", "out", "blob", "st", "idx", "used", "new_off"):
        assert not b[k].any(), k
    assert b["off"].tolist() == [0, 64, 128]


def _plane(L, b, form, ctx=True, model=M.YCOCG, elem_type=M.INT, n=16, argb=0, planes=(0, 0, 0), has_planes=True):
    """argb, planes: byte shifts of the pointers, or None for a null pointer"""
    a_ctx = b["ctx"] if ctx else None
    a_argb = None if argb is None else C.c_void_p(b["argb"].ctypes.data + argb)
    ptrs = (C.c_void_p * 3)(*[None if s is None else b["planes"][k].ctypes.data + s for k, s in enumerate(planes)])
    a_pl = ptrs if has_planes else None
    fn = getattr(L, "gf_image_" + form)
    return fn(a_ctx, model, elem_type, n, a_argb, a_pl) if form.startswith("split") else fn(a_ctx, model, elem_type, n, a_pl, a_argb)


def _reduce(L, b, form, ctx=True, width=8, height=8, factor=2, argb=0, out=0):
    a_argb = None if argb is None else C.c_void_p(b["argb"].ctypes.data + argb)
    a_out = None if out is None else C.c_void_p(b["out"].ctypes.data + out)
    return getattr(L, "gf_image_" + form)(b["ctx"] if ctx else None, width, height, factor, a_argb, a_out)


def _record(L, b, form, ctx=True, codecs=(0, 1), model=M.YCOCG, elem_type=M.SHORT, fill=-32768, grid=(12, 14, 4, 4), rect=(1, 2, 6, 8),
            has_grid=True, has_rect=True, argb=0, n_old=0, blob="blob", off="new_off", st="st", idx="idx", cap=2048):
    cod, gr, rc = np.array(codecs, np.int32), np.array(grid, np.int32), np.array(rect, np.int32)
    g = lambda k: None if k is None else _p(b[k])
    a_ctx = b["ctx"] if ctx else None
    a_argb = None if argb is None else C.c_void_p(b["argb"].ctypes.data + argb)
    a_grid, a_rect = (_p(gr) if has_grid else None), (_p(rc) if has_rect else None)
    old_blob, old_off = (g("blob"), _p(b["off"])) if n_old else (None, None)
    if form == "write_dev":
        return L.gf_image_write_dev(a_ctx, _p(cod), cod.size, model, elem_type, fill, a_grid, a_rect, a_argb, n_old, old_blob, 128 if n_old else 0,
                                    old_off, 1, 1, g(blob), cap, g(off), g(idx), _p(b["used"]), g(st))
    if form == "write":
        return L.gf_image_write(a_ctx, _p(cod), cod.size, model, elem_type, fill, a_grid, a_rect, a_argb, n_old, old_blob, old_off, 1, 1, g(blob),
                                cap, g(off), g(idx), _p(b["used"]), g(st))
    r_off = None if off is None else _p(b["off"])
    if form == "read_dev":
        return L.gf_image_read_dev(a_ctx, _p(cod), cod.size, model, elem_type, fill, a_grid, a_rect, 2, g(blob), 128, r_off, 1, a_argb, g(st))
    return L.gf_image_read(a_ctx, _p(cod), cod.size, model, elem_type, fill, a_grid, a_rect, 2, g(blob), r_off, 1, a_argb, g(st))


def test_reduce_size():
    L = _lib.lib()
    w, h = C.c_int(-7), C.c_int(-7)
    for width, height, f in ((10, 10, 1), (10, 11, 2), (4100, 4103, 2899), (21600, 10800, 60), (7, 5, 6), (5, 7, 6), (2 ** 31 - 1, 2, 2899),
                             (1, 1, 1), (2899, 2899, 2899), (16777216, 16777216, 3)):
        assert L.gf_image_reduce_size(width, height, f, C.byref(w), C.byref(h)) == OK
        assert (w.value, h.value) == M.reduce_size(width, height, f) == (width // f, height // f)
    w.value = h.value = -7
    assert L.gf_image_reduce_size(8, 8, 2, None, C.byref(h)) == ARG and L.gf_image_reduce_size(8, 8, 2, C.byref(w), None) == ARG
    for width, height, f in ((0, 8, 2), (8, 0, 2), (8, 8, 0), (-1, 8, 2), (8, -8, 2), (8, 8, -2 ** 31)):
        assert L.gf_image_reduce_size(width, height, f, C.byref(w), C.byref(h)) == ARG
    assert L.gf_image_reduce_size(8, 8, 2899, C.byref(w), C.byref(h)) == OK and (w.value, h.value) == (0, 0)
    w.value = h.value = -7
    for f in (2900, 46340, 2 ** 31 - 1):
        assert L.gf_image_reduce_size(8, 8, f, C.byref(w), C.byref(h)) == UNSUPPORTED
        assert L.gf_image_reduce_size(0, 8, f, C.byref(w), C.byref(h)) == ARG                        # ARG comes first
    assert L.gf_image_reduce_size(16777216, 16777217, 2, C.byref(w), C.byref(h)) == UNSUPPORTED      # more than 2^48 pixels
    assert (w.value, h.value) == (-7, -7)


def test_split_and_join_arguments():
    L = _lib.lib()
    b = _buffers()
    for form in PLANE:
        bad = lambda **kw: _plane(L, b, form, **kw) == ARG
        assert bad(ctx=False) and bad(argb=None) and bad(has_planes=False), form
        for k in range(3):
            assert bad(planes=tuple(None if j == k else 0 for j in range(3))), (form, k)
        for model in (-1, 2, 99):
            assert bad(model=model), (form, model)
        for t in (-1, 2, 3, 99):
            assert bad(elem_type=t), (form, t)
        assert bad(n=2 ** 48 + 1, model=2) and bad(n=2 ** 48 + 1, argb=None), form                    # ARG before UNSUPPORTED
        assert _plane(L, b, form, n=2 ** 48 + 1) == UNSUPPORTED and _plane(L, b, form, n=2 ** 63) == UNSUPPORTED, form
        assert _plane(L, b, form, n=0) == OK and _plane(L, b, form, n=0, elem_type=M.SHORT, model=M.RGB) == OK, form
        assert bad(n=0, model=5) and bad(n=0, planes=(0, None, 0)), form                              # also of nothing
    for form in ("split_dev", "join_dev"):                                                            # device pointers are aligned to their items
        bad = lambda **kw: _plane(L, b, form, **kw) == ARG
        assert bad(argb=1) and bad(argb=2) and bad(argb=3), form
        for k in range(3):
            assert bad(planes=tuple(2 if j == k else 0 for j in range(3))), (form, k)
            assert bad(planes=tuple(1 if j == k else 0 for j in range(3)), elem_type=M.SHORT), (form, k)
            assert _plane(L, b, form, planes=tuple(2 if j == k else 0 for j in range(3)), elem_type=M.SHORT, n=0) == OK, (form, k)
        assert bad(argb=2, n=0), form
    _untouched(b)


def test_reduce_arguments():
    L = _lib.lib()
    b = _buffers()
    for form in REDUCE:
        bad = lambda **kw: _reduce(L, b, form, **kw) == ARG
        assert bad(ctx=False) and bad(argb=None) and bad(out=None), form
        assert bad(width=0) and bad(height=0) and bad(factor=0) and bad(width=-8) and bad(height=-1) and bad(factor=-2), form
        assert _reduce(L, b, form, factor=2899) == OK, form                                           # an empty image: nothing to do
        assert _reduce(L, b, form, factor=2900) == UNSUPPORTED and _reduce(L, b, form, factor=2 ** 31 - 1) == UNSUPPORTED, form
        assert bad(factor=2900, width=0) and bad(factor=2900, out=None), form                         # ARG before UNSUPPORTED
        assert _reduce(L, b, form, width=16777216, height=16777217) == UNSUPPORTED, form
        assert _reduce(L, b, form, width=8, height=2, factor=3) == OK and _reduce(L, b, form, width=2, height=8, factor=3) == OK, form
    bad = lambda **kw: _reduce(L, b, "reduce_dev", **kw) == ARG
    assert bad(argb=1) and bad(argb=2) and bad(out=2) and bad(out=3)
    _untouched(b)


def test_record_form_arguments():
    L = _lib.lib()
    b = _buffers()
    for form in RECORD:
        bad = lambda **kw: _record(L, b, form, **kw) == ARG
        assert bad(ctx=False) and bad(argb=None) and bad(has_grid=False) and bad(has_rect=False) and bad(st=None), form
        for model in (-1, 2):
            assert bad(model=model), (form, model)
        for t in (-1, 2, 3):
            assert bad(elem_type=t), (form, t)
        assert bad(fill=32768) and bad(fill=-32769) and bad(fill=M.INT_MIN), form                     # a SHORT's fill is an int16
        assert not bad(fill=M.INT_MIN, elem_type=M.INT), form
        # what the block calls reject
        assert bad(rect=(1, 2, 12, 8)) and bad(rect=(1, 2, 6, 13)) and bad(rect=(-1, 2, 6, 8)) and bad(rect=(1, 2, 0, 8)), form
        assert bad(grid=(12, 14, 0, 4)) and bad(grid=(0, 14, 4, 4)), form
        assert bad(codecs=(0, 9)) and bad(blob=None) and bad(off=None), form
    for form in ("write_dev", "read_dev"):
        bad = lambda **kw: _record(L, b, form, **kw) == ARG
        assert bad(argb=2) and bad(argb=1), form
    for form in ("write_dev", "write"):
        assert _record(L, b, form, idx=None) == ARG, form
    assert _record(L, b, "write_dev", codecs=(1, 2, 0, 3)) == UNSUPPORTED                             # a list with CodecDeflate: the host form's
    assert _record(L, b, "write_dev", codecs=(1, 2, 0, 3), model=7) == ARG
    _untouched(b)


def test_valid_arguments_need_a_device():
    """what passes the checks runs with a device; without one it fails as another _dev entry point does on the same stand-in context
    (there is no CPU path behind these calls)"""
    L = _lib.lib()
    if L.gf_device_count() > 0:
        return
    b = _buffers()
    lens = np.array([64, 64], np.uint32)
    val = np.zeros((2, 16), np.int32)
    want = L.gf_huffman_decode_batch_i32_dev(b["ctx"], None, 4, 4, 2, _p(b["blob"]), 256, _p(b["off"]), 0, _p(lens), _p(val), _p(b["st"]))
    assert want < 0 and want not in (ARG, UNSUPPORTED)
    for form in PLANE:
        for model in M.MODELS:
            for et in (M.INT, M.SHORT):
                assert _plane(L, b, form, model=model, elem_type=et) == want, (form, model, et)
        assert _plane(L, b, form, n=2 ** 48) == want, form
    for form in REDUCE:
        assert _reduce(L, b, form) == want and _reduce(L, b, form, factor=8) == want, form
        assert _reduce(L, b, form, width=2899, height=2899, factor=2899) == want, form
    for form in RECORD:
        for model in M.MODELS:
            assert _record(L, b, form, model=model) == want, (form, model)
            assert _record(L, b, form, model=model, elem_type=M.INT, fill=M.INT_MIN) == want, (form, model)
        assert _record(L, b, form, codecs=()) == want, form
    assert _record(L, b, "write", codecs=(1, 2, 0, 3)) == want and _record(L, b, "read", codecs=(1, 2, 0, 3)) == want
    assert _record(L, b, "write_dev", n_old=2) == want and _record(L, b, "write", n_old=2) == want
    _untouched(b)
