"""B-spline interpolation over a grid block on the GPU (gf_block_interp_points_dev, gf_block_interp_lattice_dev and the host form):
every point of every case against the numpy model of tests/interp_ref.py, BIT FOR BIT -- the tolerance is zero -- at the smallest
shapes at which the kernels can still go wrong: a block that is the whole grid and one inside it, the fixed list of points that
takes every branch of the window rules, all targets, wraps and element types, per-point spacings with zeros, point counts around
a wave and a partly filled workgroup; lattices with every kind of step, one of several patches, each equal to the points form on
the same coordinates; every optional output left out in turn with guard words behind every array; the reference's own sample files
read as blocks and interpolated across the tile seams; the points form replayed from a hipGraph."""
import ctypes as C

import numpy as np
import pytest

import interp_cases as K
import interp_ref as R
import test_gpu_graph as TG
import test_gpu_records_elems as RE
from test_gpu_records_dev import ctx      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
OUTS = K.FIELDS + ("status",)
BAND = 256                                 # guard bytes on both sides of every output array
GRIDS = [((9, 11), None), ((12, 14), (2, 3, 7, 9))]


class Out:
    """n items (float64, 3 n for the normal, int32 for the status) in device memory between two bands of 0xA5 bytes"""

    def __init__(self, ctx, name, n):
        import gridfour_amd
        self.name, self.n = name, n
        self.nbytes = n * (24 if name == "normal" else 4 if name == "status" else 8)
        self.buf = gridfour_amd.DeviceBuffer(ctx, self.nbytes + 2 * BAND).upload(np.full(self.nbytes + 2 * BAND, 0xA5, np.uint8))
        self.ptr = self.buf.ptr.value + BAND

    def get(self):
        raw = self.buf.download(np.uint8, self.nbytes + 2 * BAND)
        assert (raw[:BAND] == 0xA5).all() and (raw[BAND + self.nbytes:] == 0xA5).all(), "guard band of %s overwritten" % self.name
        body = raw[BAND:BAND + self.nbytes].copy()
        return body.view(np.int32) if self.name == "status" else body.view(np.float64).reshape((self.n, 3) if self.name == "normal" else (self.n,))


def _up(ctx, a):
    import gridfour_amd
    a = np.ascontiguousarray(a)
    return gridfour_amd.DeviceBuffer(ctx, a.nbytes + 16).upload(a)


def _outs_of(spec, outs):
    return [k for k in (OUTS if outs is None else outs) if k != "normal" or spec.target >= R.FIRST]


def _run(ctx, spec, block, n, call, outs=None, extra=()):
    """uploads the block, allocates the guarded outputs, runs call(d_block, out pointers), downloads; what was not asked for is NaN
    (what the model has where nothing is computed)"""
    names = _outs_of(spec, outs)
    d_block = _up(ctx, block)
    o = {k: Out(ctx, k, n) for k in names}
    try:
        call(d_block.ptr, {k: v.ptr for k, v in o.items()})
        ctx.synchronize()
        got = {k: v.get() for k, v in o.items()}
    finally:
        for b in [d_block] + [v.buf for v in o.values()] + list(extra):
            b.free()
    return got


def run_points(ctx, spec, block, rows, cols, cs=None, outs=None):
    rows, cols = np.ascontiguousarray(rows, np.float64), np.ascontiguousarray(cols, np.float64)
    d_rows, d_cols = _up(ctx, rows), _up(ctx, cols)
    d_cs = None if cs is None else _up(ctx, np.ascontiguousarray(cs, np.float64))
    s = K.lib_spec(spec)
    return _run(ctx, spec, block, rows.size,
                lambda d_block, o: ctx.interp_points_dev(s, d_block, rows.size, d_rows.ptr, d_cols.ptr, o, None if d_cs is None else d_cs.ptr),
                outs, [d_rows, d_cols] + ([] if d_cs is None else [d_cs]))


def run_lattice(ctx, spec, block, lattice, cs_rows=None, outs=None):
    d_cs = None if cs_rows is None else _up(ctx, np.ascontiguousarray(cs_rows, np.float64))
    s = K.lib_spec(spec)
    return _run(ctx, spec, block, lattice[4] * lattice[5],
                lambda d_block, o: ctx.interp_lattice_dev(s, d_block, lattice, o, None if d_cs is None else d_cs.ptr),
                outs, [] if d_cs is None else [d_cs])


def _same(got, want, what=""):
    K.assert_same(got, {k: want[k] for k in got}, what)


# ---------------------------------------------------------------- 1. the points form

@pytest.mark.parametrize("wrap", [0, 1, 2])
@pytest.mark.parametrize("target", [R.VALUE, R.FIRST, R.SECOND])
def test_points_equal_the_model(ctx, target, wrap):
    rng = np.random.default_rng(300 + 10 * target + wrap)
    for (n_rows, n_cols), rect in GRIDS:
        spec = R.Spec(n_rows, n_cols, rect, R.FLOAT, wrap=wrap, target=target, row_spacing=0.37109375 + 2.0 ** -40, col_spacing=1.9 / 3.0)
        block = K.random_block(rng, R.FLOAT, spec.block[2:])
        if rect:
            block = K.float_specials(block)                               # NaN, -0.0, infinities, a subnormal among the samples
        rows, cols = K.points(rng, spec, 700)
        assert rows.size % 256 != 0                                       # the last workgroup is partly filled
        want = R.interp(spec, block, rows, cols)
        seen = set(want["status"].tolist())
        assert {R.OK, R.DECLINED, R.ERR_ARG} <= seen and (rect is None or R.ERR_BOUNDS in seen)
        _same(run_points(ctx, spec, block, rows, cols), want, (n_rows, rect))
        # per-point column spacings with zeros among them
        cs = rng.uniform(0.25, 3.0, rows.size)
        cs[::17] = 0.0
        want = R.interp(spec, block, rows, cols, cs)
        assert target == R.VALUE or (want["status"][::17] != R.OK).all()
        _same(run_points(ctx, spec, block, rows, cols, cs), want, (n_rows, rect, "spacing"))


@pytest.mark.parametrize("elem_type,fill_i", [(R.INT, -2 ** 31), (R.INT, 12345), (R.SHORT, -32768), (R.SHORT, 0), (R.ICF, 0)])
def test_every_element_type(ctx, elem_type, fill_i):
    rng = np.random.default_rng(400 + elem_type)
    for ((n_rows, n_cols), rect), wrap in zip(GRIDS, (1, 0)):
        spec = R.Spec(n_rows, n_cols, rect, elem_type, fill_i, wrap=wrap, target=R.SECOND, row_spacing=30.87, col_spacing=21.5)
        block = K.random_block(rng, elem_type, spec.block[2:], fill_i)
        rows, cols = K.points(rng, spec, 700)
        want = R.interp(spec, block, rows, cols)
        if elem_type != R.ICF:
            ok = want["status"] == R.OK
            assert np.isnan(want["z"][ok]).any() and not np.isnan(want["z"][ok]).all()      # fill cells read as NaN
        _same(run_points(ctx, spec, block, rows, cols), want, (elem_type, rect))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_point_counts_around_a_wave(ctx, n):
    rng = np.random.default_rng(500)
    spec = R.Spec(12, 14, (2, 3, 7, 9), target=R.FIRST, row_spacing=2.5, col_spacing=0.75)
    block = K.random_block(rng, R.FLOAT, (7, 9))
    rows, cols = rng.uniform(2.0, 9.0, n), rng.uniform(3.0, 12.0, n)
    _same(run_points(ctx, spec, block, rows, cols), R.interp(spec, block, rows, cols), n)


def test_host_form_equals_the_model(ctx):
    rng = np.random.default_rng(600)
    for elem_type, target in ((R.FLOAT, R.SECOND), (R.SHORT, R.VALUE), (R.INT, R.FIRST)):
        spec = R.Spec(12, 14, (2, 3, 7, 9), elem_type, -7, wrap=0, target=target, row_spacing=1.25, col_spacing=0.8)
        block = K.random_block(rng, elem_type, (7, 9), -7)
        rows, cols = K.points(rng, spec, 300)
        cs = rng.uniform(0.5, 2.0, rows.size)
        got = ctx.interp_points(K.lib_spec(spec), block, rows, cols, cs)
        want = R.interp(spec, block, rows, cols, cs)
        _same(got, want, elem_type)
        names = ["z", "status"] + (["zx", "zy", "normal"] if target >= R.FIRST else []) + (["zxx", "zxy", "zyy"] if target == R.SECOND else [])
        assert set(got) == set(names)


# ---------------------------------------------------------------- 2. the lattice form

LATTICES = [(0.3, 0.2, 0.29, 0.25, 37, 53),          # steps below 1
            (0.5, 0.5, 1.0, 1.0, 37, 53),            # equal to 1: runs off the grid
            (-0.4, -0.45, 0.31, 1.7, 37, 53),        # a start inside the fringe, a column step above 1
            (11.4, 13.3, -0.33, -0.27, 37, 53),      # negative steps
            (2.0, 3.0, 0.125, 0.125, 37, 53)]        # exact coordinates, points on the cells


@pytest.mark.parametrize("lattice", LATTICES, ids=[str(k) for k in range(len(LATTICES))])
def test_lattices_equal_the_model_and_the_points_form(ctx, lattice):
    rng = np.random.default_rng(700)
    for wrap, target, rect in ((0, R.SECOND, None), (1, R.FIRST, None), (0, R.VALUE, (2, 3, 7, 9)), (2, R.FIRST, (1, 0, 9, 14))):
        spec = R.Spec(12, 14, rect, wrap=wrap, target=target, row_spacing=0.9, col_spacing=1.1)
        block = K.random_block(rng, R.FLOAT, spec.block[2:])
        rows, cols = R.lattice_coords(*lattice)
        want = R.interp(spec, block, rows, cols)
        assert (want["status"] == R.OK).any()
        got = run_lattice(ctx, spec, block, lattice)
        _same(got, want, (wrap, target, rect))
        _same(run_points(ctx, spec, block, rows, cols), got, "points form")
        # a column spacing per lattice row, a zero among them
        cs_rows = rng.uniform(0.5, 2.0, lattice[4])
        cs_rows[5] = 0.0
        want = R.interp(spec, block, rows, cols, np.repeat(cs_rows, lattice[5]))
        _same(run_lattice(ctx, spec, block, lattice, cs_rows), want, (wrap, target, rect, "per-row spacing"))


def test_lattice_of_several_patches(ctx):
    """300 x 300 outputs: several workgroups in both directions, partial patches at the right and lower edge"""
    rng = np.random.default_rng(800)
    block = K.random_block(rng, R.SHORT, (12, 14), -32768)
    for wrap, target in ((1, R.SECOND), (0, R.VALUE)):
        spec = R.Spec(12, 14, None, R.SHORT, -32768, wrap=wrap, target=target, row_spacing=1.5, col_spacing=0.7)
        lattice = (-0.7, -1.3, 13.1 / 300, 16.9 / 300, 300, 300)
        rows, cols = R.lattice_coords(*lattice)
        want = R.interp(spec, block, rows, cols)
        got = run_lattice(ctx, spec, block, lattice)
        _same(got, want, wrap)
        _same(run_points(ctx, spec, block, rows, cols), got, "points form")
        _same(run_lattice(ctx, spec, block, lattice, np.full(300, 0.7)), got, "per-row spacing")


# ---------------------------------------------------------------- 3. optional outputs, guard words

@pytest.mark.parametrize("form", ["points", "lattice", "lattice_rows"])
def test_each_optional_output_left_out(ctx, form):
    rng = np.random.default_rng(900)
    spec = R.Spec(9, 11, target=R.SECOND, row_spacing=0.6, col_spacing=1.4)
    block = K.random_block(rng, R.FLOAT, (9, 11))
    lattice = (-0.6, -0.7, 0.41, 0.37, 27, 35)
    rows, cols = R.lattice_coords(*lattice)
    want = R.interp(spec, block, rows, cols)
    for leave in OUTS[1:] + (None,):
        outs = [k for k in OUTS if k != leave]
        if form == "points":
            got = run_points(ctx, spec, block, rows, cols, outs=outs)
        else:
            got = run_lattice(ctx, spec, block, lattice, np.full(27, 1.4) if form == "lattice_rows" else None, outs=outs)
        assert set(got) == set(outs)
        _same(got, want, leave)                                           # (Out.get has checked the guard bands)
    # outputs the target does not compute are filled with NaN
    spec = R.Spec(9, 11, target=R.VALUE)
    got = run_points(ctx, spec, block, rows, cols) if form == "points" else run_lattice(ctx, spec, block, lattice, np.full(27, 1.0) if form == "lattice_rows" else None)
    assert "normal" not in got and all(np.isnan(got[k]).all() for k in K.FIELDS[1:6])
    _same(got, R.interp(spec, block, rows, cols))


# ---------------------------------------------------------------- 4. the reference's own bytes

@pytest.mark.parametrize("name", ["Sample06_FltComp.gvrs", "Sample07_ICFComp.gvrs"])
def test_reference_samples_read_and_interpolated(golden_dir, ctx, name):
    """four 50 x 50 tiles read as one block by gf_block_read_elems_dev, then interpolated on points that straddle the tile seams;
    the model is applied to the block the read returned"""
    import gridfour_amd
    _, codecs, tile, grid, elems, verify, _ = [s for s in RE.SAMPLES if s[0] == name][0]
    master = gridfour_amd.CodecMasterHip(context=ctx) if codecs is None else gridfour_amd.CodecMasterHip(codec_list=codecs, context=ctx)
    blob, offsets, _, _ = RE._sample_blob(golden_dir, name)
    rng = np.random.default_rng(1000)
    for rect in ((0, 0, grid, grid), (tile - 3, tile - 4, 9, 11)):
        blocks, st = master.read_block_dev(tile, tile, (grid, grid), rect, blob, offsets, elems, verify_checksums=verify)
        assert (st == 0).all() and blocks[0].dtype == np.float32
        elem_type = R.FLOAT if elems[0] == "float" else R.ICF
        spec = R.Spec(grid, grid, rect, elem_type, target=R.FIRST, row_spacing=30.0, col_spacing=25.0)
        r0, c0, nr, nc = rect
        rows = np.concatenate([rng.uniform(tile - 2.5, tile + 2.5, 400), rng.uniform(r0, r0 + nr - 1, 200), [tile - 1.0, tile - 0.5, tile + 0.0] * 2])
        cols = np.concatenate([rng.uniform(tile - 2.5, tile + 2.5, 200), rng.uniform(c0, c0 + nc - 1, 200), rng.uniform(tile - 2.5, tile + 2.5, 200),
                               [tile - 1.0, tile - 0.5, tile + 0.0, tile - 0.5, tile + 0.0, tile - 1.0]])
        want = R.interp(spec, blocks[0], rows, cols)
        assert (want["status"] == R.OK).sum() > 200 and not np.isnan(want["z"][want["status"] == R.OK]).any()
        _same(run_points(ctx, spec, blocks[0], rows, cols), want, (name, rect))


# ---------------------------------------------------------------- 5. graph capture

@pytest.mark.parametrize("form", ["points", "lattice"])
def test_replayed_from_a_graph(form):
    """the device forms only enqueue: captured after one warm-up call, replayed on new coordinates and a new block"""
    import gridfour_amd
    hip = TG._hip()
    ctx = gridfour_amd.GvrsHipContext(0)
    rng = np.random.default_rng(1100)
    spec = R.Spec(12, 14, (2, 3, 7, 9), target=R.SECOND, row_spacing=0.5, col_spacing=2.0)
    lattice = (1.7, 2.6, 0.21, 0.17, 40, 70)
    n = lattice[4] * lattice[5]
    s = K.lib_spec(spec)
    d_block, d_rows, d_cols = (gridfour_amd.DeviceBuffer(ctx, nb) for nb in (7 * 9 * 4, n * 8, n * 8))
    o = {k: Out(ctx, k, n) for k in OUTS}
    ptrs = {k: v.ptr for k, v in o.items()}

    def call():
        if form == "points":
            ctx.interp_points_dev(s, d_block.ptr, n, d_rows.ptr, d_cols.ptr, ptrs)
        else:
            ctx.interp_lattice_dev(s, d_block.ptr, lattice, ptrs)

    d_block.upload(K.random_block(rng, R.FLOAT, (7, 9)))
    d_rows.upload(np.full(n, 5.0))
    d_cols.upload(np.full(n, 6.0))
    call()                                                                # warm-up outside the capture (module load)
    ctx.synchronize()
    stream = C.c_void_p(ctx.stream)
    graph, gexec = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 0) == 0
    call()
    assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and graph.value
    assert hip.hipGraphInstantiate(C.byref(gexec), graph, None, None, C.c_size_t(0)) == 0
    for k in range(2):
        block = K.random_block(rng, R.FLOAT, (7, 9))
        rows, cols = (rng.uniform(1.0, 10.0, n), rng.uniform(2.0, 13.0, n)) if form == "points" else R.lattice_coords(*lattice)
        d_block.upload(block)
        d_rows.upload(rows)
        d_cols.upload(cols)
        for v in o.values():
            v.buf.upload(np.full(v.nbytes + 2 * BAND, 0xA5, np.uint8))
        ctx.synchronize()
        assert hip.hipGraphLaunch(gexec, stream) == 0
        ctx.synchronize()
        _same({name: v.get() for name, v in o.items()}, R.interp(spec, block, rows, cols), k)
    hip.hipGraphExecDestroy(gexec)
    hip.hipGraphDestroy(graph)
