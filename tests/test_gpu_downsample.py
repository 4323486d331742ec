"""Grid blocks downsampled on the GPU (gf_block_downsample_elems_dev, its host form, gf_block_read_downsampled_elems[_dev]): every
cell of every case against the numpy model of tests/downsample_ref.py, BIT FOR BIT -- the tolerance is zero, a NaN matches any NaN,
+0.0 and -0.0 differ -- at the smallest shapes at which the kernels can still go wrong: every element type with the factors 1, 2,
3, 4, 5, 8, 16, 67 and those beside the implementation's thresholds (6, 7: the last compile-time factors of k_downsample_direct;
8 | 9: k_downsample_direct | k_downsample_staged; 2, 4, 8: one load per window row where pointer, column phase and pitch allow it),
row pitches and pointers that do and do not allow those loads, every phase of the rectangle for f = 3 and 4, trailing remainders,
outputs narrower than a wave, of 64, 256 and 257 columns, one row, one cell, staged workgroups that are partly filled.  Guard
bands of 0xA5 bytes stand on both sides of every output, and the input blocks are read back unchanged."""
import ctypes as C

import numpy as np
import pytest

import block_ref as B
import block_write_ref as W
import downsample_cases as K
import downsample_ref as R
import test_gpu_graph as TG
import test_gpu_records_elems as RE
from test_gpu_blocks import FILLS4, GRID4, TILE4, records4      # noqa: F401  (fixture)
from test_gpu_records_dev import ctx, master5      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BAND = 256                                 # guard bytes on both sides of every output
TYPES = [(R.INT, -2 ** 31), (R.SHORT, -32768), (R.FLOAT, 0)]
TYPE_IDS = ["int", "short", "float"]


def _specs(cases):
    from gridfour_amd.codec import _ELEM_SPEC
    s = np.zeros(len(cases), _ELEM_SPEC)
    for e, (elem_type, fill, _) in enumerate(cases):
        s[e]["type"], s[e]["fill_i"], s[e]["scale"] = elem_type, fill, 1.0
    return s


class Dev:
    """cases = [(elem_type, fill, values)] for one rectangle: the blocks in device memory (at `shift` bytes behind a 256-byte
    boundary) and guarded outputs for factor f"""

    def __init__(self, ctx, cases, block, f, shift=0):
        import gridfour_amd
        self.ctx, self.cases, self.block, self.f, self.shift = ctx, cases, block, f, shift
        self.out_rect = R.out_rect(block, f)
        self.n_out = self.out_rect[2] * self.out_rect[3]
        self.values = [np.ascontiguousarray(v, R.DTYPES[t]) for t, _, v in cases]
        self.d_in = [gridfour_amd.DeviceBuffer(ctx, v.nbytes + shift + 16).upload(v, shift) for v in self.values]
        self.out_bytes = [self.n_out * v.itemsize for v in self.values]
        self.d_out = [gridfour_amd.DeviceBuffer(ctx, nb + 2 * BAND) for nb in self.out_bytes]
        self.reset()

    def reset(self):
        for b, nb in zip(self.d_out, self.out_bytes):
            b.upload(np.full(nb + 2 * BAND, 0xA5, np.uint8))

    def run(self):
        self.ctx.downsample_dev(_specs(self.cases), self.block, self.f, [b.ptr.value + self.shift for b in self.d_in],
                                [b.ptr.value + BAND for b in self.d_out])

    def get(self):
        """the outputs; checks the guard bands and that the inputs are as they were"""
        outs = []
        for b, nb, v in zip(self.d_out, self.out_bytes, self.values):
            raw = b.download(np.uint8, nb + 2 * BAND)
            assert (raw[:BAND] == 0xA5).all() and (raw[BAND + nb:] == 0xA5).all(), "guard band overwritten"
            outs.append(raw[BAND:BAND + nb].copy().view(v.dtype).reshape(self.out_rect[2], self.out_rect[3]))
        for b, v in zip(self.d_in, self.values):
            assert np.array_equal(b.download(np.uint8, v.nbytes, self.shift), v.reshape(-1).view(np.uint8)), "input block changed"
        return outs

    def free(self):
        for b in self.d_in + self.d_out:
            b.free()


def run_dev(ctx, cases, block, f, shift=0):
    d = Dev(ctx, cases, block, f, shift)
    try:
        d.run()
        ctx.synchronize()
        return d.get()
    finally:
        d.free()


def _check(ctx, rng, block, f, elem_type, fill, shift=0):
    v = K.random_block(rng, block, f, elem_type, fill)
    want = R.downsample(v, block, f, elem_type, fill)
    got = run_dev(ctx, [(elem_type, fill, v)], block, f, shift)[0]
    assert R.same_bits(got, want), (block, f, elem_type, shift, np.argwhere(got.view(np.uint8).reshape(want.shape + (-1,)) !=
                                                                       want.view(np.uint8).reshape(want.shape + (-1,)))[:4])
    return want


# ---------------------------------------------------------------- 1. every factor, every type

def _block_for(f, k):
    """some 20 x 45 output cells for the small factors, 4 x 9 for f = 16, 2 x 2 for f = 67; k = 0: a rectangle on the factor's
    grid whose pitch is a multiple of 8 cells (the wide loads apply); k = 1: off the grid, a trailing remainder, an odd pitch"""
    n_out = (20, 45) if f <= 9 else (4, 9) if f <= 16 else (2, 2)
    if k == 0:
        return (2 * f, 3 * f, n_out[0] * f, (n_out[1] * f + 7) // 8 * 8)
    return (5, 3, n_out[0] * f + f - 1, (n_out[1] * f + f - 1) | 1)


@pytest.mark.parametrize("elem_type,fill", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("f", [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 67])
def test_every_factor(ctx, f, elem_type, fill):
    rng = np.random.default_rng(3000 + 10 * f + elem_type)
    for k in (0, 1):
        want = _check(ctx, rng, _block_for(f, k), f, elem_type, fill)
        if elem_type == R.FLOAT:
            assert np.isnan(want).any() and not np.isnan(want).all()
        else:
            assert (want == fill).any() and (want != fill).any()


@pytest.mark.parametrize("elem_type,fill", [(R.INT, 12345), (R.INT, 0), (R.SHORT, 0), (R.SHORT, 32767)], ids=["int", "int0", "short0", "shortmax"])
def test_other_fills(ctx, elem_type, fill):
    rng = np.random.default_rng(3500 + elem_type)
    for f in (2, 3, 9):
        _check(ctx, rng, _block_for(f, 1), f, elem_type, fill)


# ---------------------------------------------------------------- 2. where one load per window row applies, and where not

@pytest.mark.parametrize("elem_type,fill", TYPES, ids=TYPE_IDS)
def test_wide_loads_and_what_forbids_them(ctx, elem_type, fill):
    """f = 2, 4 (and 8 for SHORT): an aligned block with a pitch of 32 cells takes the wide loads; a pitch that is no multiple of
    the load (odd; 2 mod 4; 4 mod 8), a pointer 4 bytes behind a 16-byte boundary and a column phase each send some of them to the
    scalar loads: the same cells either way"""
    rng = np.random.default_rng(3600 + elem_type)
    for f in (2, 4, 8):
        for pitch in (32, 33, 34, 36, 44):
            for shift in (0, 4):
                for col0 in (0, 1, 2, 4):
                    block = (0, col0, 3 * f + 1, pitch)
                    _check(ctx, rng, block, f, elem_type, fill, shift)


# ---------------------------------------------------------------- 3. phases, remainders, widths

@pytest.mark.parametrize("elem_type,fill", TYPES, ids=TYPE_IDS)
def test_every_phase_of_the_rectangle(ctx, elem_type, fill):
    rng = np.random.default_rng(3700 + elem_type)
    for f in (3, 4):
        for row0 in range(f):
            for col0 in range(f):
                for rem in (0, f - 1):                                   # without and with trailing remainder rows and columns
                    block = (row0, col0, 4 * f + rem, 7 * f + rem)
                    want = _check(ctx, rng, block, f, elem_type, fill)
                    assert want.shape == R.out_rect(block, f)[2:] and want.shape[0] in (3, 4) and want.shape[1] in (6, 7)


@pytest.mark.parametrize("f,n_out", [(1, (3, 1)), (1, (2, 63)), (1, (2, 64)), (1, (2, 65)), (1, (2, 256)), (1, (3, 257)), (2, (2, 257)), (3, (1, 1)),
                                     (3, (1, 64)), (3, (2, 256)), (3, (1, 257)), (4, (1, 1)), (4, (1, 300)), (5, (3, 63)), (9, (1, 1)), (9, (1, 64)),
                                     (9, (2, 257)), (16, (1, 1)), (16, (2, 257)), (67, (1, 2)), (67, (1, 1)), (67, (1, 63)), (67, (3, 1))])
def test_output_widths(ctx, f, n_out):
    """outputs narrower than a wave, of exactly 64 and 256 columns and of 257, where the last workgroup is partly filled (f = 9, 16:
    k_downsample_staged takes 256 cells a workgroup; f = 67: 61 cells, so 63 are a whole workgroup and one of two cells), one output
    row, one output cell"""
    rng = np.random.default_rng(3800 + f)
    for elem_type, fill in TYPES if n_out[0] * n_out[1] * f * f < 200000 else TYPES[2:]:
        block = (f + 1, 2 * f + 1, n_out[0] * f + f - 1, n_out[1] * f + f - 1)
        assert _check(ctx, rng, block, f, elem_type, fill).shape == n_out


def test_no_whole_window_touches_nothing(ctx):
    rng = np.random.default_rng(3900)
    v = K.random_floats(rng, (1, 1, 2, 40), 1)
    got = run_dev(ctx, [(R.FLOAT, 0, v)], (1, 1, 2, 40), 3)[0]             # rows 1..2 hold no window of 3; Dev.get checked the bands
    assert got.shape == (0, 12)


# ---------------------------------------------------------------- 4. several elements, the host form, strips, a graph

def _mixed(rng, block, f):
    return [(R.FLOAT, 0, K.random_floats(rng, block, f)), (R.SHORT, -32768, K.random_ints(rng, block, f, R.SHORT, -32768)),
            (R.INT, 77, K.random_ints(rng, block, f, R.INT, 77)), (R.SHORT, 0, K.random_ints(rng, block, f, R.SHORT, 0)),
            (R.FLOAT, 0, K.random_floats(rng, block, f))]


@pytest.mark.parametrize("f", [2, 3, 9])
def test_mixed_elements_and_the_host_form(ctx, f):
    rng = np.random.default_rng(4000 + f)
    block = (7, 5, 20 * f + 1, 33 * f + 2)
    cases = _mixed(rng, block, f)
    want = [R.downsample(v, block, f, t, fill) for t, fill, v in cases]
    got = run_dev(ctx, cases, block, f)
    host = ctx.downsample(_specs(cases), block, f, [v for _, _, v in cases])
    for e in range(len(cases)):
        assert R.same_bits(got[e], want[e]), (f, e)
        assert host[e].dtype == want[e].dtype and R.same_bits(host[e], want[e]), (f, e, "host form")
    # the names of the element types and the fills of read_block_dev reach the same call
    host = ctx.downsample(["float", "short"], block, f, [cases[0][2], cases[1][2]], fills=[None, -32768])
    assert R.same_bits(host[0], want[0]) and R.same_bits(host[1], want[1])
    assert ctx.downsample_rect(block, f) == R.out_rect(block, f)


@pytest.mark.parametrize("f", [3, 4, 9])
def test_strips_give_the_cells_of_one_call(ctx, f):
    """a block worked through in strips of rows that start anywhere: each strip delivers the coarse rows whose windows it holds,
    and strips that overlap by f - 1 rows deliver every row of the single call, the same bits"""
    rng = np.random.default_rng(4100 + f)
    block = (4, 2, 61, 20 * f + 3)
    for elem_type, fill in TYPES:
        v = K.random_block(rng, block, f, elem_type, fill)
        whole = run_dev(ctx, [(elem_type, fill, v)], block, f)[0]
        assert R.same_bits(whole, R.downsample(v, block, f, elem_type, fill))
        r0, _, nr, _ = R.out_rect(block, f)
        seen = np.zeros(nr, bool)
        step = 13
        for at in range(block[0], block[0] + block[2], step):
            rows = min(step + f - 1, block[0] + block[2] - at)
            strip = (at, block[1], rows, block[3])
            sr0, _, snr, _ = R.out_rect(strip, f)
            got = run_dev(ctx, [(elem_type, fill, v[at - block[0]:at - block[0] + rows])], strip, f)[0]
            assert got.shape[0] == snr and R.same_bits(got, whole[sr0 - r0:sr0 - r0 + snr]), (f, elem_type, at)
            seen[sr0 - r0:sr0 - r0 + snr] = True
        assert seen.all()


@pytest.mark.parametrize("f", [2, 3, 9])
def test_replayed_from_a_graph(f):
    """the plain device form only enqueues: captured after one warm-up call on one stream (no branches), replayed on new blocks"""
    import gridfour_amd
    hip = TG._hip()
    ctx = gridfour_amd.GvrsHipContext(0)
    rng = np.random.default_rng(4200 + f)
    block = (1, 2, 10 * f + 2, 70 * f + 1)
    d = Dev(ctx, _mixed(rng, block, f)[:3], block, f)
    d.run()                                                               # warm-up outside the capture (module load)
    ctx.synchronize()
    stream = C.c_void_p(ctx.stream)
    graph, gexec = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 0) == 0
    d.run()
    assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and graph.value
    assert hip.hipGraphInstantiate(C.byref(gexec), graph, None, None, C.c_size_t(0)) == 0
    for k in range(2):
        cases = _mixed(rng, block, f)[:3]
        d.cases, d.values = cases, [np.ascontiguousarray(v, R.DTYPES[t]) for t, _, v in cases]
        for b, v in zip(d.d_in, d.values):
            b.upload(v)
        d.reset()
        ctx.synchronize()
        assert hip.hipGraphLaunch(gexec, stream) == 0
        ctx.synchronize()
        for e, got in enumerate(d.get()):
            assert R.same_bits(got, R.downsample(d.values[e], block, f, cases[e][0], cases[e][1])), (f, k, e)
    hip.hipGraphExecDestroy(gexec)
    hip.hipGraphDestroy(graph)
    d.free()


# ---------------------------------------------------------------- 5. tile records in, coarse blocks out

@pytest.mark.parametrize("name,codecs,tile,grid,elems,verify,fills", RE.SAMPLES, ids=[c[0][:8] for c in RE.SAMPLES])
def test_reference_samples_downsampled(golden_dir, ctx, name, codecs, tile, grid, elems, verify, fills):
    """the reference's own files, whose cells are row * nCols + col - 1: with f = 2 a window's sum is 4 * (2i * n + 2j - 1) + 2n + 2,
    so a float cell is 2in + 2j + (n - 1) / 2 exactly and an integer cell (an int-coded float's code too) floor of that + 0.5; the
    windows cross the seams of the 5 x 5 tiles.  Then f = 3 and 4 against the model on the block read's cells."""
    import gridfour_amd
    master = gridfour_amd.CodecMasterHip(context=ctx) if codecs is None else gridfour_amd.CodecMasterHip(codec_list=codecs, context=ctx)
    blob, offsets, _, _ = RE._sample_blob(golden_dir, name)
    whole = (0, 0, grid, grid)
    coarse, st = master.read_block_downsampled_dev(tile, tile, (grid, grid), whole, 2, blob, offsets, elems, verify_checksums=verify)
    assert (st == 0).all()
    i, j = np.meshgrid(np.arange(grid // 2), np.arange(grid // 2), indexing="ij")
    exact = 2.0 * i * grid + 2 * j + (grid - 1) / 2.0
    for e, el in enumerate(elems):
        if el == "float":
            assert coarse[e].dtype == np.float32 and R.same_bits(coarse[e], exact.astype(np.float32)), (name, e)
        else:
            assert coarse[e].dtype == (np.int16 if el == "short" else np.int32)
            assert np.array_equal(coarse[e], np.floor(exact + 0.5).astype(np.int64)), (name, e)
    as_int = ["int" if not isinstance(el, str) else el for el in elems]
    int_fills = [el[3] if not isinstance(el, str) else None for el in elems]
    for f, rect in ((3, whole), (4, (1, 2, grid - 1, grid - 3))):
        full, st = master.read_block_dev(tile, tile, (grid, grid), rect, blob, offsets, as_int, fills=int_fills, verify_checksums=verify)
        coarse, st2 = master.read_block_downsampled_dev(tile, tile, (grid, grid), rect, f, blob, offsets, elems, verify_checksums=verify)
        assert (st == 0).all() and np.array_equal(st, st2)
        for e, el in enumerate(as_int):
            t = {"int": R.INT, "short": R.SHORT, "float": R.FLOAT}[el]
            fill = {"int": -2 ** 31 if int_fills[e] is None else int_fills[e], "short": -32768, "float": 0}[el]
            assert R.same_bits(coarse[e], R.downsample(full[e], rect, f, t, fill)), (name, f, e)


ELEMS4_INT = ["short", "int", "float"]
FILLS4_INT = [FILLS4[0], RE.ICF3[3], FILLS4[2]]


@pytest.mark.parametrize("f", [2, 3, 7, 9])
def test_records_downsampled(master5, records4, f):
    """records of three elements (short, int-coded float, float) in shuffled order, tile 3's only record with a failing checksum
    (tests/test_gpu_blocks.py), all sixteen and the first thirteen alone, which leave tile 8 missing: the statuses are the block
    read's, the coarse blocks those of read_block_dev followed by downsample_dev, the int-coded float comes back as the codes an INT
    read of the same records averages to, and a window that touches a missing or failed tile is fill (FLOAT: the fill is averaged in)"""
    r = records4
    ctx = master5.ctx
    for n_rec, rect in ((16, (0, 0) + GRID4), (16, (13, 27, 80, 150)), (13, (0, 0) + GRID4)):
        offsets, want_st = r["offsets"][:n_rec + 1], r["st"][:, :n_rec]
        coarse, st = master5.read_block_downsampled_dev(TILE4[0], TILE4[1], GRID4, rect, f, r["blob"], offsets, RE.ELEMS3, fills=FILLS4)
        assert np.array_equal(st, want_st)
        full, st2 = master5.read_block_dev(TILE4[0], TILE4[1], GRID4, rect, r["blob"], offsets, ELEMS4_INT, fills=FILLS4_INT)
        assert np.array_equal(st2, want_st)
        cases = [(R.SHORT, FILLS4_INT[0], full[0]), (R.INT, FILLS4_INT[1], full[1]), (R.FLOAT, 0, full[2])]
        two_step = run_dev(ctx, cases, rect, f)
        host, st3 = master5.read_block_downsampled(TILE4[0], TILE4[1], GRID4, rect, f, r["blob"], offsets, RE.ELEMS3, fills=FILLS4)
        assert np.array_equal(st3, want_st)
        for e, (t, fill, v) in enumerate(cases):
            want = R.downsample(v, rect, f, t, fill)
            assert coarse[e].dtype == want.dtype and R.same_bits(coarse[e], want), (f, rect, e)
            assert R.same_bits(two_step[e], want) and R.same_bits(host[e], want), (f, rect, e)
        assert coarse[1].dtype == np.int32
    # of the first thirteen records tile 3 (rows 0..39, columns 180..199) failed and tile 8 (rows 80..99, columns 0..59) is missing
    _, _, nr, nc = R.out_rect((0, 0) + GRID4, f)
    rows, cols = (np.arange(nr) * f)[:, None], (np.arange(nc) * f)[None, :]
    touched = ((rows < 40) & (cols + f > 180)) | ((rows + f > 80) & (cols < 60))
    assert touched.any() and (coarse[0][touched] == FILLS4_INT[0]).all() and (coarse[1][touched] == FILLS4_INT[1]).all()
    inside = ((rows < 40) & (rows + f <= 40) & (cols >= 180)) | ((rows >= 80) & (cols + f <= 60))
    assert inside.any() and (coarse[2][inside] == np.float32(-7.5)).all()
    assert (coarse[0][~touched] != FILLS4_INT[0]).any() and (coarse[1][~touched] != FILLS4_INT[1]).any()


def test_records_in_overview_records_out(ctx):
    """the overview pipeline end to end: the records of a 2-element grid (INT, FLOAT) go through the block read and the downsample,
    the coarse blocks through write_block_dev on the coarse grid, and those records read back give the model: tests/block_write_ref.py
    cuts the grid, tests/block_ref.py puts it together, tests/downsample_ref.py averages, and the same two once more"""
    import gridfour_amd
    import test_gpu_block_write as TW
    grid, tile, f, ctile = (70, 90), (32, 32), 3, (8, 10)
    elems = ["int", "float"]
    master = gridfour_amd.CodecMasterHip(codec_list=[TW.HUFFMAN, TW.CANON], context=ctx)
    rs = TW.rasters(elems, grid)
    whole = (0, 0) + grid
    idx, recs, _, st = master.write_block_dev(tile[0], tile[1], grid, whole, rs, elems)
    assert (st == 0).all()
    blob, off = TW._blob(recs)
    coarse, st = master.read_block_downsampled_dev(tile[0], tile[1], grid, whole, f, blob, off, elems)
    assert (st == 0).all()
    # the model of the first half
    m_idx, m_tiles, pre = W.cut(grid, tile, whole, rs, elems)
    assert (pre == 0).all() and np.array_equal(m_idx, idx)
    m_full = [B.block_from_tiles(grid, tile, whole, m_idx, m_tiles[0], -2 ** 31),
              B.block_from_tiles(grid, tile, whole, m_idx, m_tiles[1].view(np.uint32), 0).view(np.float32)]
    m_coarse = [R.downsample(m_full[0], whole, f, R.INT, -2 ** 31), R.downsample(m_full[1], whole, f, R.FLOAT)]
    for e in range(2):
        assert R.same_bits(coarse[e], m_coarse[e]), e
    # ... and of the second
    cgrid = R.out_rect(whole, f)[2:]
    assert cgrid == (23, 30)
    cwhole = (0, 0) + cgrid
    got = master.write_block_dev(ctile[0], ctile[1], cgrid, cwhole, coarse, elems)
    want = W.expected(TW._encoder(master, ctile, elems, True, None), cgrid, ctile, cwhole, m_coarse, elems)
    TW._same(got, want, "coarse records")
    assert (got[3] == 0).all()
    cblob, coff = TW._blob(got[1])
    back, st = master.read_block_dev(ctile[0], ctile[1], cgrid, cwhole, cblob, coff, elems)
    assert (st == 0).all()
    for e in range(2):
        assert R.same_bits(back[e], m_coarse[e]), e
