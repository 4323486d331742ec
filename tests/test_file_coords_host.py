"""The host forms of the queries at coordinates, without a device: gf_file_interp_spec and gf_file_map_points against the Python
restatement coords_ref.py (every output, both directions), gf_file_interp_coords_tiles against the restatement's mapping composed
with file_points_ref.py's window tiles, every argument error the header lists, and the device entry points' answer to a NULL
context behind their argument checks."""
import ctypes as C

import numpy as np
import pytest

import gridfour_amd
from gridfour_amd import _lib
from gridfour_amd.codec import _ptr, _INTERP_OUT

import coords_cases as K
import coords_ref as CR
import file_points_ref as R

OK, ERR_ARG, ERR_NO_DEVICE = _lib.OK, _lib.ERR_ARG, _lib.ERR_NO_DEVICE


@pytest.fixture(scope="module")
def opened():
    return {name: gridfour_amd.GvrsFileHip(K.image_of(name)[0]) for name in K.GRIDS}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, want):
    """bit for bit, any NaN for a NaN the restatement gives (Python does not keep a payload apart)"""
    a, want = np.asarray(a, np.float64), np.asarray(want, np.float64)
    return bool(((bits(a) == bits(want)) | (np.isnan(a) & np.isnan(want))).all())


def test_interp_spec_of_the_case_grids(opened):
    for name, f in opened.items():
        co = CR.Coords(f.info)
        assert co.wrap == K.WRAP[name]
        for e in range(f.n_elems):
            s = f.coords_spec(e, 1)
            el = f.info["elems"][e]
            assert (int(s["elem_type"][0]), int(s["fill_i"][0]), int(s["wrap"][0]), int(s["target"][0])) == (el["type"], el["fill_i"], co.wrap, 1)
            assert s["block"][0].tolist() == [0, 0, f.grid[0], f.grid[1]]
            got = [float(s[n][0]) for n in ("row_spacing", "col_spacing", "row_fringe0", "row_fringe1", "col_fringe0", "col_fringe1")]
            assert same(got, [co.dv, co.du, co.row_fringe[0], co.row_fringe[1], co.col_fringe[0], co.col_fringe[1]]), name
    geo = CR.Coords(opened["limited"].info)
    assert geo.du == CR.R_EARTH * (3.0 * 0.017453292519943295) and geo.du > 300000


def test_map_points(opened):
    for name, f in opened.items():
        co = CR.Coords(f.info)
        x, y = K.file_points(name)
        for kind in (CR.GEO_TO_GRID, CR.MODEL_TO_GRID):
            got = f.map_points(kind, x, y)
            want = [co.map_point(kind, a, b) for a, b in zip(x.tolist(), y.tolist())]
            for k, key in enumerate(("row", "col", "irow", "icol", "col_spacing", "status")):
                w = [m[k] for m in want]
                if key in ("irow", "icol", "status"):
                    assert got[key].tolist() == w, (name, kind, key)
                else:
                    assert same(got[key], w), (name, kind, key)
            refused = got["status"] == ERR_ARG
            assert refused.any() == (name in K.GEO) and np.isnan(got["row"][refused]).all() and np.isnan(got["col_spacing"][refused]).all()
        rows, cols = K.grid_points(name)
        for kind in (CR.GRID_TO_GEO, CR.GRID_TO_MODEL):
            got = f.map_points(kind, rows, cols)
            want = [co.map_point(kind, a, b) for a, b in zip(rows.tolist(), cols.tolist())]
            assert same(got["x"], [m[0] for m in want]) and same(got["y"], [m[1] for m in want]), (name, kind)
    # the case set distinguishes the cosines through the spacing too: a libm cosine in the library would show here
    f = opened["wraps"]
    got = f.map_points(CR.GEO_TO_GRID, np.zeros(16), K.COS_TELLING)["col_spacing"]
    du = CR.Coords(f.info).du
    assert same(got, [CR.strict_cos(CR.to_radians(v)) * du for v in K.COS_TELLING])
    assert not same(got, [np.cos(CR.to_radians(v)) * du for v in K.COS_TELLING])


def test_map_points_outputs_are_optional(opened):
    L = _lib.lib()
    f = opened["wraps"]
    x, y = K.file_points("wraps")
    n = x.size
    full = f.map_points(CR.GEO_TO_GRID, x, y)
    oa, ob = np.zeros(n), np.zeros(n)
    ir = np.full(n, -7, np.int32)
    assert L.gf_file_map_points(f._h, 0, n, _ptr(x), _ptr(y), _ptr(oa), _ptr(ob), _ptr(ir), None, None, None) == OK
    assert ir.tolist() == full["irow"].tolist() and same(oa, full["row"]) and same(ob, full["col"])
    assert L.gf_file_map_points(f._h, 0, n, _ptr(x), _ptr(y), _ptr(oa), _ptr(ob), None, None, None, None) == OK
    assert L.gf_file_map_points(f._h, 0, 0, None, None, None, None, None, None, None, None) == OK


def test_interp_coords_tiles(opened):
    for name, f in opened.items():
        co = CR.Coords(f.info)
        spec = f.coords_spec(0, 1)
        ref = R.spec_of(f.grid, co.wrap, co.row_fringe, co.col_fringe)
        x, y = K.file_points(name)
        rows, cols = K.grid_points(name)
        for kind, (a, b) in ((CR.COORDS_FILE, (x, y)), (CR.COORDS_GRID, (rows, cols))):
            q = [co.query(kind, p, r) for p, r in zip(a.tolist(), b.tolist())]
            ok = np.array([s == CR.OK for s, _, _, _ in q])
            qr, qc = np.array([v[1] for v in q]), np.array([v[2] for v in q])
            want = R.windows_touched(f.grid, ref, qr[ok], qc[ok])
            got = f.interp_coords_tiles(kind, spec, a, b)
            assert got.dtype == np.int32 and got.tolist() == want.tolist(), (name, kind)
            assert want.size == len(set(range(-(-f.grid[0] // 5) * -(-f.grid[1] // 5))))       # the points cover every tile
            # one point at a time: its window's tiles alone; none for a refused point
            per_point = R.window_tiles(f.grid, ref, np.where(ok, qr, np.nan), np.where(ok, qc, np.nan))
            for i in range(0, a.size, 5):
                assert f.interp_coords_tiles(kind, spec, a[i:i + 1], b[i:i + 1]).tolist() == per_point[i], (name, kind, i)
            if name in K.GEO:
                assert (~ok).any() and all(per_point[i] == [] for i in np.nonzero(~ok)[0])
        # the grid kind without a refusal is gf_file_interp_tiles
        if name not in K.GEO:
            assert f.interp_coords_tiles(CR.COORDS_GRID, spec, rows, cols).tolist() == f.interp_tiles(spec, rows, cols).tolist()


def test_tiles_cap(opened):
    L = _lib.lib()
    f = opened["limited"]
    x, y = K.file_points("limited")
    spec = f.coords_spec(0)
    want = f.interp_coords_tiles(1, spec, x, y)
    for cap in (0, 1, want.size - 1, want.size, want.size + 2):
        tiles = np.full(want.size + 4, -7, np.int32)
        count = C.c_size_t(99)
        st = L.gf_file_interp_coords_tiles(f._h, 1, _ptr(spec), x.size, _ptr(x), _ptr(y), _ptr(tiles) if cap else None, cap, C.byref(count))
        assert st == OK and count.value == want.size
        k = min(cap, want.size)
        assert tiles[:k].tolist() == want[:k].tolist() and (tiles[k:] == -7).all()


def test_host_argument_errors(opened):
    L = _lib.lib()
    f = opened["wraps"]
    a, b, oa, ob = np.zeros(2), np.zeros(2), np.zeros(2), np.zeros(2)
    ir, ic, st, cs = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2)
    spec = f.coords_spec(0)
    out = np.zeros(1, gridfour_amd.codec._INTERP_SPEC)
    # gf_file_interp_spec
    assert L.gf_file_interp_spec(None, 0, 0, _ptr(out)) == ERR_ARG
    assert L.gf_file_interp_spec(f._h, 0, 0, None) == ERR_ARG
    for elem, target in ((-1, 0), (1, 0), (0, -1), (0, 3)):
        assert L.gf_file_interp_spec(f._h, elem, target, _ptr(out)) == ERR_ARG
    import file_points_cases as FK
    small = gridfour_amd.GvrsFileHip(FK.image_of((3, 9, 3, 3)))                  # a grid under 4 x 4
    assert L.gf_file_interp_spec(small._h, 0, 0, _ptr(out)) == ERR_ARG
    # gf_file_map_points
    good = (_ptr(a), _ptr(b), _ptr(oa), _ptr(ob))
    assert L.gf_file_map_points(None, 0, 2, *good, None, None, None, None) == ERR_ARG
    for kind in (-1, 4):
        assert L.gf_file_map_points(f._h, kind, 2, *good, None, None, None, None) == ERR_ARG
    for k in range(4):
        args = list(good)
        args[k] = None
        assert L.gf_file_map_points(f._h, 0, 2, *args, None, None, None, None) == ERR_ARG
    for kind in (2, 3):                                                          # a from-grid kind has no use for these
        for k, p in enumerate((_ptr(ir), _ptr(ic), _ptr(cs), _ptr(st))):
            extra = [None] * 4
            extra[k] = p
            assert L.gf_file_map_points(f._h, kind, 2, *good, *extra) == ERR_ARG
        assert L.gf_file_map_points(f._h, kind, 2, *good, None, None, None, None) == OK
    assert small.map_points(0, [0.0], [0.0])["status"].tolist() == [OK]          # (the mappings ask for no 4 x 4 grid)
    # gf_file_interp_coords_tiles
    tiles, n = np.zeros(4, np.int32), C.c_size_t()
    assert L.gf_file_interp_coords_tiles(None, 0, _ptr(spec), 2, _ptr(a), _ptr(b), _ptr(tiles), 4, C.byref(n)) == ERR_ARG
    assert L.gf_file_interp_coords_tiles(f._h, 0, None, 2, _ptr(a), _ptr(b), _ptr(tiles), 4, C.byref(n)) == ERR_ARG
    assert L.gf_file_interp_coords_tiles(f._h, 0, _ptr(spec), 2, None, _ptr(b), _ptr(tiles), 4, C.byref(n)) == ERR_ARG
    assert L.gf_file_interp_coords_tiles(f._h, 0, _ptr(spec), 2, _ptr(a), None, _ptr(tiles), 4, C.byref(n)) == ERR_ARG
    assert L.gf_file_interp_coords_tiles(f._h, 0, _ptr(spec), 2, _ptr(a), _ptr(b), None, 4, C.byref(n)) == ERR_ARG
    assert L.gf_file_interp_coords_tiles(f._h, 0, _ptr(spec), 2, _ptr(a), _ptr(b), _ptr(tiles), 4, None) == ERR_ARG
    for kind in (-1, 2):
        assert L.gf_file_interp_coords_tiles(f._h, kind, _ptr(spec), 2, _ptr(a), _ptr(b), _ptr(tiles), 4, C.byref(n)) == ERR_ARG
    for field, value in (("wrap", 3), ("wrap", -1), ("target", 3), ("target", -1)):
        bad = f.coords_spec(0)
        bad[field] = value
        assert L.gf_file_interp_coords_tiles(f._h, 0, _ptr(bad), 2, _ptr(a), _ptr(b), _ptr(tiles), 4, C.byref(n)) == ERR_ARG
    assert L.gf_file_interp_coords_tiles(small._h, 0, _ptr(spec), 2, _ptr(a), _ptr(b), _ptr(tiles), 4, C.byref(n)) == ERR_ARG
    assert L.gf_file_interp_coords_tiles(f._h, 0, _ptr(spec), 0, None, None, None, 0, C.byref(n)) == OK and n.value == 0


def test_device_forms_judge_their_arguments_before_the_context(opened):
    """with a NULL context every argument error is GF_ERR_ARG; with good arguments the answer is GF_ERR_NO_DEVICE on a machine
    without a device (no context can be had there) and GF_ERR_ARG where one could have been made"""
    L = _lib.lib()
    none = ERR_NO_DEVICE if L.gf_device_count() == 0 else ERR_ARG
    f = opened["wraps"]
    image = f.image
    a, b, oa, ob, z, used = (np.zeros(2) for _ in range(6))
    n = C.c_size_t()
    good = (_ptr(a), _ptr(b), _ptr(oa), _ptr(ob))
    assert L.gf_file_map_points_dev(None, f._h, 0, 2, *good, None, None, None, None) == none
    assert L.gf_file_map_points_dev(None, f._h, 4, 2, *good, None, None, None, None) == ERR_ARG
    assert L.gf_file_map_points_dev(None, f._h, 0, 2, None, _ptr(b), _ptr(oa), _ptr(ob), None, None, None, None) == ERR_ARG
    assert L.gf_file_map_points_dev(None, f._h, 2, 2, *good, None, None, _ptr(used), None) == ERR_ARG
    assert L.gf_file_map_points_dev(None, None, 0, 2, *good, None, None, None, None) == ERR_ARG
    spec = f.coords_spec(0, 1)
    out = np.zeros(1, _INTERP_OUT)
    out["z"] = z.ctypes.data
    for name in ("gf_file_interp_coords_dev", "gf_file_interp_coords"):
        fn = getattr(L, name)

        def call(elem=0, kind=1, sp=spec, pa=a, o=out, img=image, size=image.size, pn=n, cs=None):
            return fn(None, f._h, _ptr(img) if img is not None else None, size, elem, kind, _ptr(sp) if sp is not None else None, 2,
                      _ptr(pa) if pa is not None else None, _ptr(b), None if cs is None else _ptr(cs), 1, 4, _ptr(o) if o is not None else None,
                      _ptr(used), C.byref(pn) if pn is not None else None)
        assert call() == none
        assert call(cs=used) == none                                             # col_spacing_used beside the caller's spacings: a source
        assert call(elem=1) == ERR_ARG and call(elem=-1) == ERR_ARG
        assert call(kind=2) == ERR_ARG and call(kind=-1) == ERR_ARG
        assert call(sp=None) == ERR_ARG and call(pa=None) == ERR_ARG and call(o=None) == ERR_ARG and call(img=None) == ERR_ARG
        assert call(pn=None) == ERR_ARG and call(size=8) == ERR_ARG
        assert call(o=np.zeros(1, _INTERP_OUT)) == ERR_ARG                       # out->z is required
        for field, value in (("wrap", 3), ("target", 3), ("row_spacing", 0.0), ("col_spacing", 0.0)):
            bad = f.coords_spec(0, 1)
            bad[field] = value
            assert call(sp=bad) == ERR_ARG, field
        bad = f.coords_spec(0, 1)
        bad["col_spacing"] = 0.0
        assert call(sp=bad, cs=used) == none                                     # (per-point spacings: a zero col_spacing is not looked at)
        value = f.coords_spec(0, 0)
        with_normal = np.zeros(1, _INTERP_OUT)
        with_normal["z"], with_normal["normal"] = z.ctypes.data, z.ctypes.data
        assert call(sp=value, o=with_normal) == ERR_ARG                          # normal with target VALUE
        assert fn(None, None, None, 0, 0, 0, None, 2, None, None, None, 1, 4, None, None, None) == ERR_ARG
    if L.gf_device_count() == 0:
        assert L.gf_file_interp_coords_dev(None, f._h, _ptr(image[1:]), image.size - 1, 0, 1, _ptr(spec), 2, _ptr(a), _ptr(b), None, 1, 4, _ptr(out),
                                           None, C.byref(n)) == ERR_ARG          # an unaligned d_image


def test_read_coords_needs_no_new_entry_point(opened):
    """GvrsElement.readValue(GridPoint) is the mapping's integers handed to the existing cell read: the tiles they touch"""
    f = opened["cart"]
    x, y = K.file_points("cart")
    m = f.map_points(CR.MODEL_TO_GRID, x, y)
    inside = (m["irow"] >= 0) & (m["irow"] < 9) & (m["icol"] >= 0) & (m["icol"] < 11)
    assert inside.any() and (~inside).any()
    assert f.cells_tiles(m["irow"], m["icol"]).tolist() == R.cells_touched(f.grid, m["irow"], m["icol"]).tolist()
