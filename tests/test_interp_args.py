"""CPU-only: gf_block_interp_points_dev, gf_block_interp_lattice_dev and gf_block_interp_points reject what the host can check with
GF_ERR_ARG / GF_ERR_UNSUPPORTED before the context or a device is looked at (host memory stands in for both and stays untouched);
n_points == 0 is GF_OK; without a device valid arguments fail as the other _dev entry points do."""
import ctypes as C

import numpy as np

import gridfour_amd
from gridfour_amd import _lib
from gridfour_amd.codec import _INTERP_LATTICE, _INTERP_OUT

FORMS = ("points_dev", "lattice_dev", "points")
OUTS = ("z", "zx", "zy", "zxx", "zxy", "zyy", "normal", "status")


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _buffers():
    fake = C.create_string_buffer(8192)
    b = dict(ctx=C.cast(fake, C.c_void_p), keep=fake, blk=np.zeros(12 * 14, np.float32), rows=np.full(8, 5.0), cols=np.full(8, 6.0),
             cs=np.full(8, 2.0))
    for k in OUTS:
        b[k] = np.zeros(8 * 3, np.float64) if k != "status" else np.zeros(8, np.int32)
    return b


def _call(L, b, form, ctx="ctx", spec=True, block="blk", n=8, rows="rows", cols="cols", cs=None, out=True, outs=("z", "status"), lattice=(0.5, 0.5, 1.0, 1.0, 2, 4),
          **spec_args):
    g = lambda k: None if k is None else (b[k] if k == "ctx" else _p(b[k]))
    args = dict(n_rows_grid=12, n_cols_grid=14, block=None, elem_type="float", target=0)
    args.update(spec_args)
    args["block"] = args.pop("rect", None)
    s = gridfour_amd.interp_spec(**args)                                # (alive during the call, as o and lat)
    o = np.zeros(1, _INTERP_OUT)
    for k in outs:
        o[k] = b[k].ctypes.data
    ps, po = (_p(s) if spec else None), (_p(o) if out else None)
    if form == "points_dev":
        return L.gf_block_interp_points_dev(g(ctx), None, ps, g(block), n, g(rows), g(cols), g(cs), po)
    if form == "points":
        return L.gf_block_interp_points(g(ctx), ps, g(block), n, g(rows), g(cols), g(cs), po)
    lat = np.zeros(1, _INTERP_LATTICE)
    if lattice is not None:
        lat["row0"], lat["col0"], lat["row_step"], lat["col_step"], lat["n_rows"], lat["n_cols"] = lattice
    return L.gf_block_interp_lattice_dev(g(ctx), None, ps, g(block), _p(lat) if lattice is not None else None, g(cs), po)


def _untouched(b):
    for k in OUTS:
        assert (b[k] == 0).all(), k
    assert (b["blk"] == 0).all() and (b["rows"] == 5.0).all() and (b["cols"] == 6.0).all() and (b["cs"] == 2.0).all()


def test_arguments_are_checked_before_the_device():
    L = _lib.lib()
    b = _buffers()
    for form in FORMS:
        bad = lambda **kw: _call(L, b, form, **kw) == _lib.ERR_ARG
        assert bad(ctx=None) and bad(spec=False) and bad(block=None) and bad(out=False), form
        assert bad(outs=("zx", "status")), form                                               # out->z is null
        # a grid under 4 x 4; a block under 4 x 4, outside the grid, beyond 32 bits
        assert bad(n_rows_grid=3, rect=(0, 0, 3, 4)) and bad(n_cols_grid=3, rect=(0, 0, 4, 3)) and bad(n_rows_grid=-5), form
        for rect in ((0, 0, 3, 14), (0, 0, 12, 3), (-1, 0, 5, 5), (0, -1, 5, 5), (9, 0, 4, 4), (0, 11, 4, 4), (0, 0, 13, 14), (0, 0, 12, 15),
                     (2 ** 31 - 1, 0, 2 ** 31 - 1, 4), (0, 2 ** 31 - 1, 4, 2 ** 31 - 1), (0, 0, 0, 0), (0, 0, -4, 4)):
            assert bad(rect=rect), (form, rect)
        for t in (-1, 4, 99):
            assert bad(elem_type=t), (form, t)
        for w in (-1, 3):
            assert bad(wrap=w), (form, w)
        for t in (-1, 3):
            assert bad(target=t), (form, t)
        assert bad(elem_type="short", fill_i=32768) and bad(elem_type="short", fill_i=-32769), form
        # zero spacings with derivatives asked for; a per-point / per-row spacing array stands in for a zero col_spacing only
        for t in (1, 2):
            assert bad(target=t, row_spacing=0.0) and bad(target=t, col_spacing=0.0) and bad(target=t, row_spacing=0.0, cs="cs"), (form, t)
        assert bad(target=0, outs=("z", "normal")), form                                      # a normal needs first derivatives
    for form in ("points_dev", "points"):
        assert _call(L, b, form, rows=None) == _lib.ERR_ARG and _call(L, b, form, cols=None) == _lib.ERR_ARG, form
    assert _call(L, b, "lattice_dev", lattice=None) == _lib.ERR_ARG
    for lat in ((0, 0, 1, 1, 0, 4), (0, 0, 1, 1, 4, 0), (0, 0, 1, 1, -1, 4), (0, 0, 1, 1, 4, -2 ** 40)):
        assert _call(L, b, "lattice_dev", lattice=lat) == _lib.ERR_ARG, lat
    _untouched(b)


def test_lattice_limit_is_unsupported():
    L = _lib.lib()
    b = _buffers()
    for lat in ((0, 0, 1, 1, 2 ** 32, 2 ** 31), (0, 0, 1, 1, 2 ** 62, 2), (0, 0, 1, 1, 2 ** 63 - 1, 2 ** 63 - 1)):
        assert _call(L, b, "lattice_dev", lattice=lat) == _lib.ERR_UNSUPPORTED, lat
        assert _call(L, b, "lattice_dev", lattice=lat, wrap=7) == _lib.ERR_ARG                 # the argument checks come first
    _untouched(b)


def test_no_points_is_ok():
    L = _lib.lib()
    b = _buffers()
    for form in ("points_dev", "points"):
        assert _call(L, b, form, n=0) == _lib.OK and _call(L, b, form, n=0, rows=None, cols=None) == _lib.OK
        assert _call(L, b, form, n=0, wrap=5) == _lib.ERR_ARG
    _untouched(b)


def test_valid_arguments_need_a_device():
    """what passes the checks runs with a device; without one it fails as another _dev entry point does on the same stand-in
    context (there is no CPU path behind these calls)"""
    L = _lib.lib()
    if L.gf_device_count() > 0:
        return
    b = _buffers()
    blob, off, lens = np.zeros(256, np.uint8), np.array([0, 64, 128], np.uint64), np.array([64, 64], np.uint32)
    val, st = np.zeros((2, 16), np.int32), np.zeros(2, np.int32)
    want = L.gf_huffman_decode_batch_i32_dev(b["ctx"], None, 4, 4, 2, _p(blob), blob.size, _p(off), 0, _p(lens), _p(val), _p(st))
    assert want < 0
    for form in FORMS:
        assert _call(L, b, form) == want, form
        assert _call(L, b, form, rect=(8, 10, 4, 4), wrap=2) == want, form                    # touches the grid's last row and column
        assert _call(L, b, form, target=2, outs=OUTS, col_spacing=0.0, cs="cs") == want, form
        assert _call(L, b, form, elem_type="short", fill_i=-32768) == want, form
    assert _call(L, b, "lattice_dev", lattice=(0, 0, 1, 1, 2 ** 31, 2 ** 31)) == want          # 2^62 points: allowed by the checks
    _untouched(b)
