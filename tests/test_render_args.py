"""CPU-only: gf_palette_create and the gf_block_render_* entry points reject what the host can check with GF_ERR_ARG /
GF_ERR_UNSUPPORTED before the context or a device is looked at (host memory stands in for both and stays untouched); n == 0 is
GF_OK; without a device valid arguments fail as the other _dev entry points do.  The palette's host half -- checks, the stable sort,
the hinge, the records' deltas, the packed table -- is seen through gf_internal_palette_create_host / gf_internal_palette_table
(not part of the public ABI): the table equals the model's byte for byte, and a lookup on it shows the sort."""
import ctypes as C

import numpy as np

import gridfour_amd
from gridfour_amd import _lib
from gridfour_amd.codec import _INTERP_LATTICE, _RENDER_OUT

import render_cases as RC
import render_ref as M

FORMS = ("lattice_dev", "points_dev", "points_dev_lattice", "lattice")
RGB1 = [(0.0, 1.0, "rgb", (1, 2, 3), (4, 5, 6))]


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _internals():
    L = _lib.lib()
    L.gf_internal_palette_create_host.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.gf_internal_palette_create_host.restype = C.c_int
    L.gf_internal_palette_table.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.gf_internal_palette_table.restype = C.c_int
    return L


def _create(L, fn, ctx, spec=True, out=True, records=RGB1, n_records=None, null_records=False, **kw):
    """gf_palette_create (fn "device", on the stand-in context) or its host half (fn "host") -> (status, handle)"""
    s, recs = gridfour_amd.palette_spec(records, **kw)
    if n_records is not None:
        s["n_records"] = n_records
    if null_records:
        s["records"] = 0
    h = C.c_void_p(0x5a5a)
    ph = C.byref(h) if out else None
    if fn == "host":
        return L.gf_internal_palette_create_host(_p(s) if spec else None, ph), h
    return L.gf_palette_create(ctx, _p(s) if spec else None, ph), h


def _table(L, h):
    n = C.c_size_t(0)
    assert L.gf_internal_palette_table(h, None, 0, C.byref(n)) == _lib.ERR_CAPACITY
    buf = np.zeros(n.value, np.uint8)
    assert L.gf_internal_palette_table(h, _p(buf), buf.size, C.byref(n)) == _lib.OK
    return buf.tobytes()


def test_palette_arguments_are_checked_before_the_device():
    L = _internals()
    fake = C.create_string_buffer(8192)
    ctx = C.cast(fake, C.c_void_p)
    many = RC._ramp(257)
    for fn in ("device", "host"):
        bad = lambda want=_lib.ERR_ARG, **kw: _create(L, fn, ctx, **kw)[0] == want
        assert bad(spec=False) and bad(out=False) and bad(null_records=True) and bad(n_records=0) and bad(n_records=-3), fn
        for r0, r1 in ((1.0, 0.5), (np.nan, 1.0), (0.0, np.nan), (np.nan, np.nan), (np.inf, -np.inf)):
            assert bad(records=RGB1 + [(r0, r1, "rgb", (0, 0, 0), (0, 0, 0))]), (fn, r0, r1)
        for model in (-1, 2, 99):
            assert bad(records=[(0.0, 1.0, model, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))]), (fn, model)
        for c0, c1 in (((256, 0, 0), (0, 0, 0)), ((0, -1, 0), (0, 0, 0)), ((0, 0, 0), (0, 0, 256)), ((0, 0, 0), (-2 ** 31, 0, 0))):
            assert bad(records=[(0.0, 1.0, "rgb", c0, c1)]), (fn, c0, c1)
        two = [(0.0, 1.0, "rgb", (1, 2, 3), (4, 5, 6)), (1.0, 2.0, "rgb", (1, 2, 3), (4, 5, 6))]
        assert bad(records=two, hinge=True, hinge_value=0.5) and bad(records=two, hinge=True, hinge_value=np.nan), fn
        assert bad(records=two, hinge=True, hinge_value=0.0, normalized=True, range_max=1.0), fn       # the hinge on the first record
        assert bad(_lib.ERR_UNSUPPORTED, records=many), fn
        assert bad(records=many + [(3.0, 2.0, "rgb", (0, 0, 0), (0, 0, 0))]) and bad(records=many, hinge=True, hinge_value=0.123), fn   # ARG comes first
    assert _create(L, "device", None)[0] == _lib.ERR_ARG                  # a NULL context
    # what the checks let through: the host half succeeds, an HSV record's channels are not range-checked
    for kw in (dict(records=RC._ramp(256)), dict(records=two, hinge=True, hinge_value=1.0, normalized=True, range_max=1.0),
               dict(records=two, hinge=True, hinge_value=0.0), dict(records=[(0.0, 0.0, "hsv", (720.0, -1.0, 9.0), (-5.0, 2.0, np.nan))]),
               dict(records=[(-np.inf, np.inf, "rgb", (0, 0, 0), (255, 255, 255))])):
        st, h = _create(L, "host", None, **kw)
        assert st == _lib.OK and h.value not in (None, 0x5a5a), kw
        L.gf_palette_destroy(h)
    assert bytes(fake.raw) == bytes(8192)
    L.gf_palette_destroy(None)


def test_the_packed_table_equals_the_models():
    """sort, keys, hinge index, RGB deltas, the HSV constructor's rules and wrap-around: every byte"""
    L = _internals()
    for name in sorted(RC.PALETTES):
        st, h = _create(L, "host", None, **RC.lib_palette_args(name))
        assert st == _lib.OK, name
        assert _table(L, h) == RC.pack_table(RC.model(name)), name
        L.gf_palette_destroy(h)


def test_the_sort_is_stable_seen_through_a_lookup(tmp_path):
    """three records with the same range, then -0.0 against 0.0: the table keeps the caller's order among equals, and the record a
    lookup lands on (the CPU harness on the library's table) is the one Java's stable sort and binary search give"""
    L = _internals()
    exe = RC.build_harness()
    same = [(0.0, 1.0, "rgb", (k, 0, 0), (k, 0, 0)) for k in (7, 3, 9)]
    mixed = [(0.0, 1.0, "rgb", (1, 0, 0), (1, 0, 0)), (-0.0, 1.0, "rgb", (2, 0, 0), (2, 0, 0)), (0.0, 0.5, "rgb", (3, 0, 0), (3, 0, 0))]
    for recs, z, want in ((same, [0.0, 0.5], [0xff030000, 0xff090000]),            # key found at mid = 1; 0.5: the record before index 3
                          (mixed, [-0.0, 0.0, 0.25, 0.75], [0xff020000, 0xff030000, 0xff010000, 0xff010000])):
        st, h = _create(L, "host", None, records=recs)
        assert st == _lib.OK
        table = _table(L, h)
        L.gf_palette_destroy(h)
        pal = M.Palette(recs)
        assert table == RC.pack_table(pal)
        assert pal.argb(z).tolist() == want
        assert RC.harness_lookup(exe, str(tmp_path), table, np.array(z)).tolist() == want


# ---------------------------------------------------------------- the render entry points

def _buffers(L):
    fake = C.create_string_buffer(8192)
    st, pal = _create(L, "host", None, **RC.lib_palette_args("etopo1"))
    assert st == _lib.OK
    return dict(ctx=C.cast(fake, C.c_void_p), keep=fake, pal=pal, blk=np.zeros(12 * 14, np.float32), rows=np.full(8, 5.0), cols=np.full(8, 6.0),
                cs=np.full(8, 2.0), argb=np.zeros(8, np.int32), shade=np.zeros(8, np.float64), status=np.zeros(8, np.int32),
                light=gridfour_amd.render_light(-2.0, 2.0, (0.0, 0.6, 0.8), 0.25))


def _call(L, b, form, ctx="ctx", spec=True, block="blk", pal="pal", light="light", flags=0, out=True, outs=("argb", "status"), n=8, rows="rows",
          cols="cols", cs=None, lattice=(0.5, 0.5, 1.0, 1.0, 2, 4), **spec_args):
    g = lambda k: None if k is None else (b[k] if k in ("ctx", "pal") else _p(b[k]))
    args = dict(n_rows_grid=12, n_cols_grid=14, block=None, elem_type="float", target=0)
    args.update(spec_args)
    args["block"] = args.pop("rect", None)
    s = gridfour_amd.interp_spec(**args)
    o = np.zeros(1, _RENDER_OUT)
    for k in outs:
        o[k] = b[k].ctypes.data
    ps, po = (_p(s) if spec else None), (_p(o) if out else None)
    lat = None
    if lattice is not None:
        lat = np.zeros(1, _INTERP_LATTICE)
        lat["row0"], lat["col0"], lat["row_step"], lat["col_step"], lat["n_rows"], lat["n_cols"] = lattice
    if form == "lattice_dev":
        return L.gf_block_render_lattice_dev(g(ctx), None, ps, g(block), _p(lat), g(pal), g(light), flags, po)
    if form == "lattice":
        return L.gf_block_render_lattice(g(ctx), ps, g(block), _p(lat), g(pal), g(light), flags, po)
    if form == "points_dev_lattice":
        return L.gf_block_render_points_dev(g(ctx), None, ps, g(block), _p(lat), 0, None, None, g(cs), g(pal), g(light), flags, po)
    return L.gf_block_render_points_dev(g(ctx), None, ps, g(block), None, n, g(rows), g(cols), g(cs), g(pal), g(light), flags, po)


def _cells(L, b, ctx="ctx", pal="pal", flags=0, elem_type=2, fill_i=0, cells="blk", n=8, shade=None, argb="argb", offsets=(0, 0, 0)):
    g = lambda k, off=0: None if k is None else (b[k] if k in ("ctx", "pal") else C.c_void_p(b[k].ctypes.data + off))
    return L.gf_block_render_cells_dev(g(ctx), None, g(pal), flags, elem_type, fill_i, g(cells, offsets[0]), n, g(shade, offsets[1]), g(argb, offsets[2]))


def _untouched(b):
    assert (b["argb"] == 0).all() and (b["shade"] == 0).all() and (b["status"] == 0).all() and (b["blk"] == 0).all()
    assert (b["rows"] == 5.0).all() and (b["cols"] == 6.0).all() and (b["cs"] == 2.0).all()


def test_render_arguments_are_checked_before_the_device():
    L = _internals()
    b = _buffers(L)
    for form in FORMS:
        bad = lambda **kw: _call(L, b, form, **kw) == _lib.ERR_ARG
        assert bad(ctx=None) and bad(spec=False) and bad(block=None) and bad(out=False) and bad(pal=None), form
        assert bad(outs=("status",)) and bad(outs=()), form                                  # neither argb nor shade
        assert bad(light=None, outs=("argb", "shade")) and bad(light=None, outs=("shade",)), form   # a shade output needs a light
        for flags in (2, -1, 1 << 16, 3):
            assert bad(flags=flags), (form, flags)
        # the interpolator's catalogue
        assert bad(n_rows_grid=3, rect=(0, 0, 3, 4)) and bad(n_cols_grid=3, rect=(0, 0, 4, 3)) and bad(n_rows_grid=-5), form
        for rect in ((0, 0, 3, 14), (0, 0, 12, 3), (-1, 0, 5, 5), (0, -1, 5, 5), (9, 0, 4, 4), (0, 11, 4, 4), (0, 0, 13, 14), (0, 0, 12, 15),
                     (2 ** 31 - 1, 0, 2 ** 31 - 1, 4), (0, 2 ** 31 - 1, 4, 2 ** 31 - 1), (0, 0, 0, 0), (0, 0, -4, 4)):
            assert bad(rect=rect), (form, rect)
        for t in (-1, 4, 99):
            assert bad(elem_type=t), (form, t)
        for w in (-1, 3):
            assert bad(wrap=w), (form, w)
        for t in (-1, 3):
            assert bad(target=t) and bad(target=t, light=None), (form, t)
        assert bad(elem_type="short", fill_i=32768) and bad(elem_type="short", fill_i=-32769), form
        # with a light first derivatives are evaluated, whatever the spec's target: zero spacings are refused; without one they are not looked at
        assert bad(row_spacing=0.0) and bad(col_spacing=0.0), form
        if form.startswith("points_dev"):
            assert bad(row_spacing=0.0, cs="cs"), form
    for lat in ((0, 0, 1, 1, 0, 4), (0, 0, 1, 1, 4, 0), (0, 0, 1, 1, -1, 4), (0, 0, 1, 1, 4, -2 ** 40)):
        for form in ("lattice_dev", "lattice", "points_dev_lattice"):
            assert _call(L, b, form, lattice=lat) == _lib.ERR_ARG, (form, lat)
    for form in ("lattice_dev", "lattice"):
        assert _call(L, b, form, lattice=None) == _lib.ERR_ARG, form
    assert _call(L, b, "points_dev", rows=None) == _lib.ERR_ARG and _call(L, b, "points_dev", cols=None) == _lib.ERR_ARG
    # a lattice and coordinate arrays at once
    lat = np.zeros(1, _INTERP_LATTICE)
    lat["n_rows"], lat["n_cols"] = 2, 4
    s, o = gridfour_amd.interp_spec(12, 14), np.zeros(1, _RENDER_OUT)
    o["argb"] = b["argb"].ctypes.data
    assert L.gf_block_render_points_dev(b["ctx"], None, _p(s), _p(b["blk"]), _p(lat), 8, _p(b["rows"]), _p(b["cols"]), None, b["pal"], None, 0,
                                        _p(o)) == _lib.ERR_ARG
    # the cells form
    bad = lambda **kw: _cells(L, b, **kw) == _lib.ERR_ARG
    assert bad(ctx=None) and bad(pal=None) and bad(cells=None) and bad(argb=None)
    for flags in (2, -1, 3):
        assert bad(flags=flags), flags
    for t in (-1, 5):
        assert bad(elem_type=t), t
    assert bad(elem_type=1, fill_i=32768) and bad(elem_type=1, fill_i=-32769)
    assert bad(offsets=(2, 0, 0)) and bad(offsets=(1, 0, 0), elem_type=1) and bad(offsets=(0, 4, 0), shade="shade") and bad(offsets=(0, 0, 2))
    assert bad(offsets=(4, 0, 0), elem_type=gridfour_amd.RENDER_Z, cells="shade")              # doubles at an odd word
    assert _cells(L, b, n=2 ** 48 + 1) == _lib.ERR_UNSUPPORTED and _cells(L, b, n=2 ** 48 + 1, flags=8) == _lib.ERR_ARG
    _untouched(b)
    L.gf_palette_destroy(b["pal"])


def test_limits_and_empty_calls():
    L = _internals()
    b = _buffers(L)
    for lat in ((0, 0, 1, 1, 2 ** 32, 2 ** 31), (0, 0, 1, 1, 2 ** 62, 2), (0, 0, 1, 1, 2 ** 63 - 1, 2 ** 63 - 1)):
        for form in ("lattice_dev", "lattice", "points_dev_lattice"):
            assert _call(L, b, form, lattice=lat) == _lib.ERR_UNSUPPORTED, (form, lat)
            assert _call(L, b, form, lattice=lat, wrap=7) == _lib.ERR_ARG                      # the argument checks come first
    assert _call(L, b, "points_dev", n=0) == _lib.OK and _call(L, b, "points_dev", n=0, rows=None, cols=None) == _lib.OK
    assert _call(L, b, "points_dev", n=0, wrap=5) == _lib.ERR_ARG and _call(L, b, "points_dev", n=0, pal=None) == _lib.ERR_ARG
    assert _cells(L, b, n=0) == _lib.OK and _cells(L, b, n=0, cells=None, argb=None) == _lib.OK and _cells(L, b, n=0, elem_type=7) == _lib.ERR_ARG
    _untouched(b)
    L.gf_palette_destroy(b["pal"])


def test_valid_arguments_need_a_device():
    """what passes the checks runs with a device; without one it fails as another _dev entry point does on the same stand-in
    context (there is no CPU path behind these calls)"""
    L = _internals()
    if L.gf_device_count() > 0:
        return
    b = _buffers(L)
    blob, off, lens = np.zeros(256, np.uint8), np.array([0, 64, 128], np.uint64), np.array([64, 64], np.uint32)
    val, st = np.zeros((2, 16), np.int32), np.zeros(2, np.int32)
    want = L.gf_huffman_decode_batch_i32_dev(b["ctx"], None, 4, 4, 2, _p(blob), blob.size, _p(off), 0, _p(lens), _p(val), _p(st))
    assert want < 0
    for form in FORMS:
        assert _call(L, b, form) == want, form
        assert _call(L, b, form, light=None, row_spacing=0.0, col_spacing=0.0, flags=1) == want, form    # no light: spacings are not looked at
        assert _call(L, b, form, outs=("argb", "shade", "status"), rect=(8, 10, 4, 4), wrap=2, target=2) == want, form
        assert _call(L, b, form, outs=("shade",), elem_type="short", fill_i=-32768) == want, form
    assert _call(L, b, "points_dev", col_spacing=0.0, cs="cs") == want and _call(L, b, "points_dev_lattice", col_spacing=0.0, cs="cs") == want
    assert _cells(L, b) == want and _cells(L, b, shade="shade", flags=1, elem_type=1, fill_i=-5) == want and _cells(L, b, offsets=(4, 8, 4)) == want
    assert _cells(L, b, elem_type=gridfour_amd.RENDER_Z, cells="shade", shade="cs") == want
    fake = C.create_string_buffer(8192)
    st, h = _create(L, "device", C.cast(fake, C.c_void_p))
    assert st == want and not h.value
    _untouched(b)
    L.gf_palette_destroy(b["pal"])
