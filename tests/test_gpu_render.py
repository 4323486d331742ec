"""Grid blocks rendered to ARGB on the GPU (gf_palette_create, gf_block_render_cells_dev, gf_block_render_lattice_dev,
gf_block_render_points_dev and the host form): every word of every case against the numpy model of tests/render_ref.py, BIT FOR BIT
-- the tolerance is zero -- at the smallest shapes that reach every seam of the kernels: cell counts around a group of four and a
workgroup at every alignment of input and output, all element types and palettes; lattices around both patch seams with every kind
of step, wrap and status; the fused kernel against interpolation followed by the cells form; the per-row-spacing lattice against
the points form; the reference's own sample file; a replay from a hipGraph.  Every output array lies between guard bands."""
import ctypes as C

import numpy as np
import pytest

import interp_cases as K
import interp_ref as R
import render_cases as RC
import render_ref as M
import scratch_plan as sp
import test_gpu_graph as TG
import test_gpu_interp as TI
import test_gpu_records_elems as RE
from test_gpu_records_dev import ctx      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
GUARD = 0xA5A5A5A5


def _palette(ctx, name):
    import gridfour_amd
    return gridfour_amd.Palette(ctx, **RC.lib_palette_args(name))


def _words(out, lead, n):
    """the n words behind `lead` spare ones of an Out made for more: the spare words on both sides still hold the guard pattern"""
    raw = out.get().view(np.uint32)
    assert (raw[:lead] == GUARD).all() and (raw[lead + n:] == GUARD).all(), "words beside the output overwritten"
    return raw[lead:lead + n]


# ---------------------------------------------------------------- 1. the cells form

SIZES = (1, 3, 4, 5, 255, 256, 257, 1031)
ELEMS = ((R.INT, np.int32, 12345), (R.SHORT, np.int16, -32768), (R.FLOAT, np.float32, 0), (R.ICF, np.float32, 0))


def _cell_pool(pal, elem_type, dtype, fill, rng):
    """the boundary set of the header test as cells of the element: float32 values (with their own neighbours), or integers
    around every edge with fill cells among them"""
    z = RC.lookup_z(pal, rng, 300)
    if elem_type in (R.FLOAT, R.ICF):
        with np.errstate(all="ignore"):
            f = z.astype(np.float32)
        return np.concatenate([f, np.nextafter(f[300:], np.float32(-np.inf)), np.nextafter(f[300:], np.float32(np.inf))])
    lim = 2.0 ** 15 if elem_type == R.SHORT else 2.0 ** 31
    v = np.round(z[np.isfinite(z)])
    v = np.concatenate([v, v - 1, v + 1, [fill] * 9])
    return rng.permutation(np.clip(v, -lim, lim - 1)).astype(dtype)


def _run_cells(ctx, pal, elem_type, cells, in_skew, out_skew, fill=0, shades=None, unlimited=False):
    """cells behind in_skew spare items, argb behind out_skew spare words"""
    n = cells.size
    d_cells = TI._up(ctx, np.concatenate([np.zeros(in_skew, cells.dtype), cells]))
    d_shade = None if shades is None else TI._up(ctx, np.concatenate([np.zeros(1), shades]))
    out = TI.Out(ctx, "status", n + 4)
    try:
        ctx.render_cells_dev(pal, elem_type, d_cells.ptr.value + in_skew * cells.itemsize, n, out.ptr + 4 * out_skew,
                             None if d_shade is None else d_shade.ptr.value + 8, fill, unlimited)
        ctx.synchronize()
        return _words(out, out_skew, n)
    finally:
        for b in [d_cells, out.buf] + ([] if d_shade is None else [d_shade]):
            b.free()


@pytest.mark.parametrize("name", ["one", "two_equal_keys", "etopo1", "categorical", "gaps_256", "hinge", "hsv", "point_records"])
def test_cells_equal_the_model(ctx, name):
    """palettes of 1, 2, 41, 3, 256, 8 (normalised with a hinge), 8 (HSV) and 4 records"""
    rng = np.random.default_rng(2000)
    model, pal = RC.model(name), _palette(ctx, name)
    k = 0
    for elem_type, dtype, fill in ELEMS:
        pool = _cell_pool(model, elem_type, dtype, fill, rng)
        for n in SIZES:
            cells = np.resize(np.roll(pool, -37 * k), n)
            in_skew, out_skew = k % 4 if elem_type != R.SHORT else k % 5, (k // 2) % 4      # 4- / 2-byte steps: aligned and misaligned starts
            shades = RC.shades_for(rng, n) if k % 3 else None
            unlimited = bool(k % 2)
            want = M.render_cells(model, cells, elem_type, fill, shades, unlimited)
            got = _run_cells(ctx, pal, elem_type, cells, in_skew, out_skew, fill, shades, unlimited)
            assert np.array_equal(got, want), (name, elem_type, n, in_skew, out_skew, shades is not None, unlimited, np.flatnonzero(got != want)[:8])
            k += 1
        # the largest size once more in each of the four forms, 16-byte aligned on both sides
        cells = np.resize(pool, SIZES[-1])
        shades = RC.shades_for(rng, cells.size)
        for sh, unlimited in ((None, False), (None, True), (shades, False), (shades, True)):
            want = M.render_cells(model, cells, elem_type, fill, sh, unlimited)
            assert np.array_equal(_run_cells(ctx, pal, elem_type, cells, 0, 0, fill, sh, unlimited), want), (name, elem_type, unlimited)
        if elem_type in (R.INT, R.SHORT):
            assert (cells == fill).any()
    pal.close()


def test_cells_take_doubles(ctx):
    """elem_type RENDER_Z: the boundary set itself, every double of it"""
    import gridfour_amd
    rng = np.random.default_rng(2100)
    for name in ("etopo1", "hinge", "hsv"):
        model, pal = RC.model(name), _palette(ctx, name)
        z = RC.lookup_z(model, rng, 300)
        sh = RC.shades_for(rng, z.size)
        for skew, shades, unlimited in ((0, None, False), (1, sh, True), (3, sh, False)):
            got = _run_cells(ctx, pal, gridfour_amd.RENDER_Z, z, 0, skew, 0, shades, unlimited)
            assert np.array_equal(got, model.argb(z, shades, unlimited)), (name, skew)
        pal.close()


# ---------------------------------------------------------------- 2. the lattice form

SHAPES = [(1, 1), (16, 64), (17, 65), (33, 130)]
# (grid of TI.GRIDS, wrap, light, unlimited, outputs, (row0, col0, row_step, col_step) as functions of the shape)
LATTICE_CASES = [
    (0, 0, "extract", False, ("argb", "shade", "status"), lambda nr, nc: (-0.9, -2.6, 10.4 / nr, 16.2 / nc)),           # fractional steps; beyond the fringe
    (1, 0, "cog", True, ("argb", "status"), lambda nr, nc: (1.7, 2.6, 8.1 / nr, 10.3 / nc)),                            # the inner block: ERR_BOUNDS around it
    (0, 1, "cog", False, ("argb",), lambda nr, nc: (8.4, 12.9, -9.1 / nr, -15.7 / nc)),                                 # negative steps, wrapped columns
    (0, 2, None, False, ("argb", "status"), lambda nr, nc: (3.25, -3.4 if nc > 1 else 4.75, 0.0, 17.3 / nc)),           # a zero row step; no light
    (1, 1, "extract", False, ("shade", "status"), lambda nr, nc: (np.nan if nr == 1 else 4.5, 5.5, 0.125, 0.0)),        # a zero column step; no argb
]


def _run_render(ctx, spec, block, n, call, outs):
    d_block = TI._up(ctx, block)
    o = {k: TI.Out(ctx, "status" if k == "argb" else k, n) for k in outs}
    try:
        call(d_block.ptr, {k: v.ptr for k, v in o.items()})
        ctx.synchronize()
        got = {k: v.get() for k, v in o.items()}
    finally:
        for b in [d_block] + [v.buf for v in o.values()]:
            b.free()
    if "argb" in got:
        got["argb"] = got["argb"].view(np.uint32)
    return got


def _assert_render(got, want, what):
    for k, v in got.items():
        assert (R.same_bits(v, want[k]) if k == "shade" else np.array_equal(v, want[k])), (what, k)


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_lattices_equal_the_model_and_the_unfused_path(ctx, shape):
    import gridfour_amd
    rng = np.random.default_rng(2200)
    n_rows, n_cols = shape
    model = M.Palette(RC._ramp(9, -70.0, 70.0, gaps=True), 0xff00ff00)    # the samples of K.random_block lie in -128 .. 128
    pal = gridfour_amd.Palette(ctx, RC._ramp(9, -70.0, 70.0, gaps=True), 0xff00ff00)
    seen = set()
    for g, wrap, light_name, unlimited, outs, start in LATTICE_CASES:
        (grid, rect), light = TI.GRIDS[g], (RC.LIGHTS[light_name] if light_name else None)
        spec = R.Spec(grid[0], grid[1], rect, R.FLOAT, wrap=wrap, target=R.SECOND, row_spacing=0.37109375 + 2.0 ** -40, col_spacing=1.9 / 3.0)
        block = K.float_specials(K.random_block(rng, R.FLOAT, spec.block[2:])) if g == 0 and wrap == 0 else K.random_block(rng, R.FLOAT, spec.block[2:])
        lattice = start(n_rows, n_cols) + (n_rows, n_cols)
        rows, cols = R.lattice_coords(*lattice)
        want = M.render_points(spec, block, rows, cols, model, light, unlimited=unlimited)
        seen |= set(want["status"].tolist())
        s, li = K.lib_spec(spec), RC.lib_light(light)
        got = _run_render(ctx, spec, block, rows.size, lambda d_block, o: ctx.render_lattice_dev(s, d_block, lattice, pal, o, li, unlimited), outs)
        assert set(got) == set(outs)
        _assert_render(got, want, (shape, g, wrap, light_name))
        if "argb" not in outs:
            continue
        # fused equals unfused: gf_block_interp_lattice_dev's z through the cells form, with the model's shade
        z = TI.run_lattice(ctx, s_model(spec, light), block, lattice, outs=["z"])["z"]
        unfused = _run_cells(ctx, pal, gridfour_amd.RENDER_Z, z, 0, 0, 0, want.get("shade"), unlimited)
        assert np.array_equal(unfused, got["argb"]), (shape, g, wrap, "unfused")
    assert seen >= {R.OK, R.DECLINED, R.ERR_BOUNDS, R.ERR_ARG}, seen       # every interpolation status occurs
    pal.close()


def s_model(spec, light):
    """the model's Spec with the target the render evaluates"""
    import copy
    s = copy.copy(spec)
    s.target = R.FIRST if light is not None else R.VALUE
    return s


def test_host_form_equals_the_model(ctx):
    rng = np.random.default_rng(2300)
    import gridfour_amd
    model, pal = RC.model("hsv"), _palette(ctx, "hsv")
    for elem_type, fill, light in ((R.SHORT, -7, RC.LIGHTS["cog"]), (R.INT, 3, None)):
        spec = R.Spec(12, 14, (2, 3, 7, 9), elem_type, fill, row_spacing=1.25, col_spacing=0.8)
        block = (K.random_block(rng, elem_type, (7, 9), fill).astype(np.int64) % 90 - 10).astype(np.int16 if elem_type == R.SHORT else np.int32)
        lattice = (2.2, 3.1, 0.23, 0.11, 21, 67)
        rows, cols = R.lattice_coords(*lattice)
        want = M.render_points(spec, block, rows, cols, model, light)
        got = ctx.render_lattice(K.lib_spec(spec), block, lattice, pal, RC.lib_light(light))
        assert set(got) == {"argb", "status"} | ({"shade"} if light else set())
        assert all(v.shape == (21, 67) for v in got.values())
        got = {k: v.ravel() for k, v in got.items()}
        got["argb"] = got["argb"].view(np.uint32)
        _assert_render(got, want, elem_type)
        assert (want["argb"] != model.argb_for_null).sum() > 100
    pal.close()


# ---------------------------------------------------------------- 3. per-row spacings and point lists

@pytest.mark.parametrize("n", [63, 64, 65, 700])
def test_row_spacings_and_points_agree(ctx, n):
    """a lattice of n points with a column spacing per row (zeros among them), the same coordinates as a point list with the
    spacing repeated per point: equal to each other and to the model"""
    import gridfour_amd
    rng = np.random.default_rng(2400 + n)
    model, pal = RC.model("hsv"), _palette(ctx, "hsv")
    n_rows, n_cols = (7, n // 7) if n % 7 == 0 else (1, n) if n == 65 else (n // 8, 8) if n % 8 == 0 else (3, n // 3)
    assert n_rows * n_cols == n
    for g, (elem_type, fill), light_name, unlimited in ((0, (R.FLOAT, 0), "extract", False), (1, (R.INT, 5), "cog", True), (1, (R.SHORT, -9), None, False)):
        (grid, rect), light = TI.GRIDS[g], (RC.LIGHTS[light_name] if light_name else None)
        spec = R.Spec(grid[0], grid[1], rect, elem_type, fill, wrap=0, row_spacing=2.5, col_spacing=0.75)
        block = K.random_block(rng, elem_type, spec.block[2:], fill)
        if elem_type != R.FLOAT:
            block = (block.astype(np.int64) % 90 - 10).astype(block.dtype)      # inside the palette's range
            block[block == fill] += 1
            block.reshape(-1)[[0, 31]] = fill                                   # two fill cells: NaN samples in some windows
        lattice = (-0.8, -0.9, (grid[0] + 0.7) / n_rows, (grid[1] + 0.9) / n_cols, n_rows, n_cols) if g == 0 else \
                  (1.2, 2.3, 7.1 / n_rows, 8.9 / n_cols, n_rows, n_cols)        # (around the inner block)
        if n_rows == 1:
            lattice = (4.3,) + lattice[1:]                                      # (the one row inside)
        rows, cols = R.lattice_coords(*lattice)
        cs_rows = rng.uniform(0.25, 3.0, n_rows)
        cs_rows[::3] = 0.0 if n_rows > 1 else cs_rows[0]
        cs = np.repeat(cs_rows, n_cols)
        want = M.render_points(spec, block, rows, cols, model, light, cs, unlimited)
        if light is not None and n_rows > 1:
            assert (want["status"].reshape(n_rows, n_cols)[::3] != R.OK).all()          # the interpolator's GF_ERR_ARG for a zero spacing
        s, li = K.lib_spec(spec), RC.lib_light(light)
        outs = ("argb", "status") + (("shade",) if light else ())
        d_cs_rows, d_cs, d_rows, d_cols = (TI._up(ctx, a) for a in (cs_rows, cs, rows, cols))
        by_rows = _run_render(ctx, spec, block, n, lambda d_block, o: ctx.render_points_dev(s, d_block, pal, o, lattice=lattice, d_col_spacing=d_cs_rows.ptr,
                                                                                          light=li, unlimited=unlimited), outs)
        by_points = _run_render(ctx, spec, block, n, lambda d_block, o: ctx.render_points_dev(s, d_block, pal, o, n_points=n, d_rows=d_rows.ptr, d_cols=d_cols.ptr,
                                                                                            d_col_spacing=d_cs.ptr, light=li, unlimited=unlimited), outs)
        for b in (d_cs_rows, d_cs, d_rows, d_cols):
            b.free()
        _assert_render(by_rows, want, (n, g, "rows"))
        _assert_render(by_points, by_rows, (n, g, "points"))
        ok = want["status"] == R.OK
        assert ok.any() and (want["argb"] != model.argb_for_null).any() and (want["argb"][~ok] == model.argb_for_null).all()
    pal.close()


# ---------------------------------------------------------------- 4. the reference's own bytes

def test_reference_sample_rendered_across_the_tile_seams(golden_dir, ctx):
    """four 50 x 50 tiles of Sample06_FltComp.gvrs read as one block by gf_block_read_elems_dev, rendered with ETOPO1.cpt
    normalised to the block's range, on a lattice that straddles the seams; the model is applied to the block the read returned"""
    import gridfour_amd
    name = "Sample06_FltComp.gvrs"
    _, codecs, tile, grid, elems, verify, _ = [s for s in RE.SAMPLES if s[0] == name][0]
    master = gridfour_amd.CodecMasterHip(context=ctx)
    blob, offsets, _, _ = RE._sample_blob(golden_dir, name)
    rect = (tile - 20, tile - 21, 40, 43)
    blocks, st = master.read_block_dev(tile, tile, (grid, grid), rect, blob, offsets, elems, verify_checksums=verify)
    assert (st == 0).all() and blocks[0].dtype == np.float32
    block = blocks[0]
    lo, hi = float(np.nanmin(block)), float(np.nanmax(block))
    assert hi > lo
    args = RC.cpt("ETOPO1.cpt", normalized=True, range_min=lo, range_max=hi)
    model, pal = M.Palette(**args), gridfour_amd.Palette(ctx, **args)
    spec = R.Spec(grid, grid, rect, R.FLOAT, row_spacing=30.0, col_spacing=25.0)
    light = M.Light(-50.0, 50.0, RC.LIGHTS["extract"].sun, 0.2)
    lattice = (tile - 18.5, tile - 19.25, 35.0 / 70, 38.0 / 150, 70, 150)
    rows, cols = R.lattice_coords(*lattice)
    want = M.render_points(spec, block, rows, cols, model, light)
    assert (want["status"] == R.OK).all() and len(set(want["argb"].tolist())) > 50 and (want["argb"] != model.argb_for_null).sum() > 5000
    s = K.lib_spec(spec)
    got = _run_render(ctx, spec, block, rows.size, lambda d_block, o: ctx.render_lattice_dev(s, d_block, lattice, pal, o, RC.lib_light(light)),
                      ("argb", "shade", "status"))
    _assert_render(got, want, name)
    pal.close()


# ---------------------------------------------------------------- 5. graph capture

def test_lattice_replayed_from_a_graph():
    """the device form only enqueues: captured after one warm-up call, replayed on new blocks; the context's scratch stays put"""
    import gridfour_amd
    hip = TG._hip()
    ctx = gridfour_amd.GvrsHipContext(0)
    rng = np.random.default_rng(2500)
    args = dict(records=RC._ramp(9, -70.0, 70.0, gaps=True), argb_for_null=0xff00ff00)
    model, pal = M.Palette(**args), gridfour_amd.Palette(ctx, **args)
    light = RC.LIGHTS["extract"]
    spec = R.Spec(12, 14, (2, 3, 7, 9), row_spacing=0.5, col_spacing=2.0)
    lattice = (1.7, 2.6, 0.21, 0.17, 40, 70)
    n = lattice[4] * lattice[5]
    rows, cols = R.lattice_coords(*lattice)
    s, li = K.lib_spec(spec), RC.lib_light(light)
    d_block = gridfour_amd.DeviceBuffer(ctx, 7 * 9 * 4 + 16)
    o = {k: TI.Out(ctx, "status" if k == "argb" else k, n) for k in ("argb", "shade", "status")}
    ptrs = {k: v.ptr for k, v in o.items()}
    call = lambda: ctx.render_lattice_dev(s, d_block.ptr, lattice, pal, ptrs, li)
    d_block.upload(K.random_block(rng, R.FLOAT, (7, 9)))
    call()                                                                # warm-up outside the capture (module load)
    ctx.synchronize()
    scratch = sp.context_scratch(ctx)
    stream = C.c_void_p(ctx.stream)
    graph, gexec = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 0) == 0
    call()
    assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and graph.value
    assert hip.hipGraphInstantiate(C.byref(gexec), graph, None, None, C.c_size_t(0)) == 0
    for k in range(2):
        block = K.random_block(rng, R.FLOAT, (7, 9))
        d_block.upload(block)
        for v in o.values():
            v.buf.upload(np.full(v.nbytes + 2 * TI.BAND, 0xA5, np.uint8))
        ctx.synchronize()
        assert hip.hipGraphLaunch(gexec, stream) == 0
        ctx.synchronize()
        got = {name: v.get() for name, v in o.items()}
        got["argb"] = got["argb"].view(np.uint32)
        _assert_render(got, M.render_points(spec, block, rows, cols, model, light), k)
    assert sp.context_scratch(ctx) == scratch                             # sizes, total bytes and moves of the context's buffers
    hip.hipGraphExecDestroy(gexec)
    hip.hipGraphDestroy(graph)
    pal.close()
    ctx.close()
