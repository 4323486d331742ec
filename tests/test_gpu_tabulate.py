"""Grid blocks tabulated on the GPU (gf_block_tabulate_dense[_dev], gf_block_tabulate_symbols[_dev]): every counter, every table
entry and every scalar of every case against the numpy model of tests/tabulate_ref.py, BIT FOR BIT -- min / max are compared as
bit patterns, +0.0 and -0.0 differ -- at the smallest shapes at which the kernels can still go wrong.  The sizes come from the
implementation's thresholds, read out of gvrs_tabulate_common.h by tests/tabulate_cases.py.  Guard bands of 0xA5 bytes stand on both
sides of every output, the outputs themselves are pre-filled with 0xA5, and the input blocks are read back unchanged."""
import ctypes as C

import numpy as np
import pytest

import tabulate_cases as K
import tabulate_ref as R
import test_gpu_blocks as TB
import test_gpu_records_elems as RE
from test_gpu_blocks import records4      # noqa: F401  (fixture)
from test_gpu_records_dev import ctx, master5      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BAND = 256                                 # guard bytes on both sides of every output
TYPES = [R.INT, R.SHORT, R.FLOAT]
TYPE_IDS = ["int", "short", "float"]
NAMES = {R.INT: "int", R.SHORT: "short", R.FLOAT: "float"}


class Guarded:
    """nbytes of device memory, pre-filled with 0xA5, between two guard bands"""

    def __init__(self, ctx, nbytes):
        import gridfour_amd
        self.nbytes = int(nbytes)
        self.buf = gridfour_amd.DeviceBuffer(ctx, self.nbytes + 2 * BAND)
        self.buf.upload(np.full(self.nbytes + 2 * BAND, 0xA5, np.uint8))

    @property
    def ptr(self):
        return C.c_void_p(self.buf.ptr.value + BAND)

    def get(self, dtype):
        raw = self.buf.download(np.uint8, self.nbytes + 2 * BAND)
        assert (raw[:BAND] == 0xA5).all() and (raw[BAND + self.nbytes:] == 0xA5).all(), "guard band overwritten"
        return raw[BAND:BAND + self.nbytes].copy().view(dtype)

    def free(self):
        self.buf.free()


class Block:
    """cells in device memory, `shift` bytes behind a 256-byte boundary"""

    def __init__(self, ctx, values, shift=0):
        import gridfour_amd
        self.values, self.shift = values, shift
        self.buf = gridfour_amd.DeviceBuffer(ctx, values.nbytes + shift + 16)
        if values.size:
            self.buf.upload(values, shift)

    def ptr(self, first=0):
        return C.c_void_p(self.buf.ptr.value + self.shift + first * self.values.itemsize)

    def unchanged(self):
        v = self.values
        return v.size == 0 or np.array_equal(self.buf.download(np.uint8, v.nbytes, self.shift), v.reshape(-1).view(np.uint8))

    def free(self):
        self.buf.free()


def dense_dev(ctx, elem_type, values, window, fill_i=0, skip_fill=False, shift=0, strips=None, first_cell=0):
    """(counter, summary) of gf_block_tabulate_dense_dev; strips = [(a, b), ...]: one call per strip of cells, the first one
    initialising, the others accumulating with first_cell = first_cell + a"""
    from gridfour_amd.codec import TAB_SUMMARY
    v = np.ascontiguousarray(values, R.DTYPES[elem_type]).ravel()
    n_bins = R.plan(*window)["n_bins"]
    blk, cnt, summ = Block(ctx, v, shift), Guarded(ctx, n_bins * 4), Guarded(ctx, TAB_SUMMARY.itemsize)
    try:
        for k, (a, b) in enumerate(strips or [(0, v.size)]):
            ctx.tabulate_dense_dev(elem_type, blk.ptr(a), b - a, *window, cnt.ptr, summ.ptr, fill_i=fill_i, skip_fill=skip_fill, accumulate=k > 0,
                                   first_cell=first_cell + a)
        ctx.synchronize()
        assert blk.unchanged(), "input block changed"
        return cnt.get(np.int32), K.summary_dict(summ.get(TAB_SUMMARY))
    finally:
        for x in (blk, cnt, summ):
            x.free()


def check_dense(ctx, elem_type, values, window, **kw):
    got = dense_dev(ctx, elem_type, values, window, **kw)
    model_kw = {k: v for k, v in kw.items() if k in ("fill_i", "skip_fill", "first_cell")}
    want = R.dense(values, elem_type, *window, **model_kw)
    assert np.array_equal(got[0], want[0]), (elem_type, len(values), window, kw, np.flatnonzero(got[0] != want[0])[:8])
    assert R.same_summary(got[1], want[1]), (elem_type, len(values), window, kw, got[1], want[1])
    return want


def symbols_dev(ctx, elem_type, values, cap):
    """(symbols [cap], counts [cap], summary) of gf_block_tabulate_symbols_dev, the tables whole"""
    from gridfour_amd.codec import TAB_SYMBOLS
    v = np.ascontiguousarray(values, R.DTYPES[elem_type]).ravel()
    blk, sym, cnt, summ = Block(ctx, v), Guarded(ctx, cap * 4), Guarded(ctx, cap * 4), Guarded(ctx, TAB_SYMBOLS.itemsize)
    try:
        ctx.tabulate_symbols_dev(elem_type, blk.ptr(), v.size, sym.ptr if cap else None, cnt.ptr if cap else None, cap, summ.ptr)
        ctx.synchronize()
        assert blk.unchanged(), "input block changed"
        s = summ.get(TAB_SYMBOLS)
        return sym.get(np.uint32), cnt.get(np.int32), {k: s[k][0].item() for k in TAB_SYMBOLS.names}
    finally:
        for x in (blk, sym, cnt, summ):
            x.free()


def check_symbols(ctx, elem_type, values, cap=None):
    want_sym, want_cnt, want = R.symbols(values, elem_type)
    cap = want["n_symbols"] + 3 if cap is None else cap
    sym, cnt, s = symbols_dev(ctx, elem_type, values, cap)
    want = dict(want, n_written=min(want["n_symbols"], cap))
    assert s == want, (elem_type, len(values), cap, s, want)
    n = want["n_written"]
    assert np.array_equal(sym[:n], want_sym[:n]) and np.array_equal(cnt[:n], want_cnt[:n]), (elem_type, len(values), cap)
    assert (sym[n:] == 0xA5A5A5A5).all() and (cnt[n:].view(np.uint32) == 0xA5A5A5A5).all(), "table written behind n_written"
    return want_sym, want_cnt, want


# ---------------------------------------------------------------- dense form: sizes, heads and tails of the wide loads

@pytest.mark.parametrize("elem_type", TYPES, ids=TYPE_IDS)
def test_dense_sizes(ctx, elem_type):
    """1, 63, 64, 65 cells, one workgroup's first trip - 1, itself and + 1, two workgroups, and one size beyond one trip of the whole
    grid of persistent workgroups"""
    rng = np.random.default_rng(400 + elem_type)
    trip = K.first_trip(elem_type)
    sizes = [1, 63, 64, 65, trip - 1, trip, trip + 1, 2 * trip + 5, K.MAX_GROUPS * trip + 3 * trip + 7]
    whole = K.dem_like(rng, sizes[-1], elem_type)
    for n in sizes:
        want = check_dense(ctx, elem_type, whole[:n], K.REF_RANGE, first_cell=3 * n)
        assert want[1]["n_cells"] == n
    assert want[1]["n_samples"] < n and want[0].max() > 1                  # samples outside the window; bins with several samples


@pytest.mark.parametrize("elem_type", TYPES, ids=TYPE_IDS)
def test_dense_heads_and_tails(ctx, elem_type):
    """blocks that start 0, 4, 8 and 12 bytes behind a 16-byte boundary, with every count up to three loads' worth and some more:
    the cells in front of the first whole load and behind the last one (a SHORT block with an odd count among them)"""
    rng = np.random.default_rng(500 + elem_type)
    per = K.cells_per_load(elem_type)
    whole = K.dem_like(rng, 3 * K.first_trip(elem_type), elem_type, -300, 500)
    for shift in (0, 4, 8, 12):
        for n in list(range(1, 3 * per + 2)) + [K.first_trip(elem_type) + per + 1, 2 * K.first_trip(elem_type) + 3]:
            check_dense(ctx, elem_type, whole[shift:shift + n], (-300, 500, 1.0), shift=shift)


# ---------------------------------------------------------------- dense form: the table's size

@pytest.mark.parametrize("n_bins", [1, 2, K.LDS_MAX_BINS - 1, K.LDS_MAX_BINS, K.LDS_MAX_BINS + 1, 19652], ids=lambda b: "bins%d" % b)
def test_dense_table_sizes(ctx, n_bins):
    """tables of 1 and 2 counters, the LDS threshold - 1, itself and + 1 (the last one takes global atomics) and the reference's
    19,652: every bin hit exactly once (+ samples on both sides of the window), and every cell in one bin"""
    rng = np.random.default_rng(n_bins)
    window = K.window(n_bins, def_min=10)
    assert R.plan(*window)["n_bins"] == n_bins
    once = rng.permutation(np.arange(8, 10 + n_bins + 2, dtype=np.int32))                          # two below, two above
    want = check_dense(ctx, R.INT, once, window)
    assert (want[0] == 1).all() and want[1]["n_samples"] == n_bins == once.size - 4
    last = 10 + n_bins - 1
    want = check_dense(ctx, R.INT, np.full(3 * K.first_trip(R.INT) + 1, last, np.int32), window)
    assert want[0][-1] == 3 * K.first_trip(R.INT) + 1 and want[0].sum() == want[0][-1] and want[1]["min_at"] == 0 == want[1]["max_at"]
    if n_bins <= 65536:
        short = (once[:60000] - 20000).astype(np.int16)
        check_dense(ctx, R.SHORT, short, K.window(n_bins, def_min=-19990))


def test_dense_outside_and_around_the_window(ctx):
    """samples below and above the window, and samples so far from it that sample - base wraps back into it: at scale 2 the window
    2^30 - 50 .. 2^30 + 99 has base 2^31 - 100 and 301 counters, so its upper part lies beyond 2^31 and belongs to samples near -2^31"""
    window = (2 ** 30 - 50, 2 ** 30 + 99, 2.0)
    w = np.array([2 ** 30 - 50, 2 ** 30 - 1, 2 ** 30 - 51, -2 ** 30 + 5, -2 ** 30 + 99, -2 ** 30 + 100, 0, 2 ** 30, -2 ** 30, 2 ** 31 - 1, -2 ** 31],
                 np.int32)
    lit = R.dense_literal(w, R.INT, *window)
    assert lit[0].size == 301 and lit[0][[0, 98, 99, 100, 101, 111, 299]].tolist() == [1, 1, 2, 1, 1, 1, 1] and lit[1]["n_samples"] == 8
    want = check_dense(ctx, R.INT, np.tile(w, 700), window)
    assert np.array_equal(want[0], 700 * lit[0]) and want[1]["n_samples"] == 5600
    f = np.tile(K.float_edge_block(), 300)
    want = check_dense(ctx, R.FLOAT, f, K.REF_RANGE)
    assert want[0][19650] == 300 and want[0][19651] == 600 and want[0][1] == 300 and want[0][0] == 300 and want[1]["n_skipped"] == 300
    assert want[1]["min"] == -np.inf and want[1]["max"] == np.inf and want[1]["min_at"] == 1 and want[1]["max_at"] == 0


@pytest.mark.parametrize("scale", [0.9, 0.7, 0.35])
def test_dense_scale_went_through_a_float(ctx, scale):
    v = K.scale_trap_block()
    window = (0, int(v.max()), scale)
    want = check_dense(ctx, R.INT, v, window)
    assert not np.array_equal(want[0], R.dense(v, R.INT, *window, scale_used=scale)[0])            # the double scale would bin otherwise
    check_dense(ctx, R.SHORT, v[v < 32768], window)
    check_dense(ctx, R.FLOAT, v.astype(np.float32) * np.float32(0.5), window)


@pytest.mark.parametrize("elem_type", [R.INT, R.SHORT], ids=["int", "short"])
def test_dense_global_atomics_with_a_scale(ctx, elem_type):
    """a table above the LDS threshold with a scale that is not 1: int cells through the FP64 sample into global atomics"""
    rng = np.random.default_rng(650 + elem_type)
    v = K.dem_like(rng, 2 * K.first_trip(elem_type) + 13, elem_type, -300, 30000)
    for scale in (0.9, 2.5):
        window = (-300, int((K.LDS_MAX_BINS + 500) / scale), scale)
        assert R.plan(*window)["n_bins"] > K.LDS_MAX_BINS
        want = check_dense(ctx, elem_type, v, window)
        assert want[1]["n_samples"] > v.size // 4 and np.count_nonzero(want[0]) > 50
        check_dense(ctx, elem_type, K.scale_trap_block()[:6000].astype(R.DTYPES[elem_type]), window)


# ---------------------------------------------------------------- dense form: what is a sample; min / max and their ties

@pytest.mark.parametrize("elem_type", [R.INT, R.SHORT], ids=["int", "short"])
def test_dense_skip_fill(ctx, elem_type):
    """the fill is the would-be minimum: skipped it is no sample at all, not skipped it is the minimum"""
    rng = np.random.default_rng(600 + elem_type)
    fill = -32768 if elem_type == R.SHORT else -2 ** 31
    v = K.dem_like(rng, 2 * K.first_trip(elem_type) + 11, elem_type)
    v[rng.random(v.size) < 0.1] = fill
    v[[0, v.size - 1]] = fill
    skipped = check_dense(ctx, elem_type, v, K.REF_RANGE, fill_i=fill, skip_fill=True)
    kept = check_dense(ctx, elem_type, v, K.REF_RANGE, fill_i=fill, skip_fill=False)
    other = check_dense(ctx, elem_type, v, K.REF_RANGE, fill_i=fill + 1, skip_fill=True)
    assert skipped[1]["n_skipped"] == int((v == fill).sum()) > 2 and skipped[1]["min"] > fill
    assert kept[1]["n_skipped"] == 0 and kept[1]["min"] == fill and kept[1]["min_at"] == 0 and other[1]["min"] == fill
    assert skipped[1]["sum_i"] != kept[1]["sum_i"]
    check_dense(ctx, elem_type, np.full(70, fill, R.DTYPES[elem_type]), K.REF_RANGE, fill_i=fill, skip_fill=True)      # no sample at all


def test_dense_float_ignores_skip_fill(ctx):
    v = np.array([0.0, 1.0, 2.0, 0.0], np.float32)
    got = dense_dev(ctx, R.FLOAT, v, (0, 5, 1.0), fill_i=0, skip_fill=True)
    want = R.dense(v, R.FLOAT, 0, 5, 1.0)
    assert np.array_equal(got[0], want[0]) and R.same_summary(got[1], want[1]) and got[1]["n_skipped"] == 0


def test_dense_no_sample_at_all(ctx):
    for n in (1, 64, K.first_trip(R.FLOAT) + 5):
        want = check_dense(ctx, R.FLOAT, np.full(n, np.nan, np.float32), K.REF_RANGE)
        assert want[1]["min"] == np.inf and want[1]["max"] == -np.inf and want[1]["min_at"] == -1 == want[1]["max_at"] and want[1]["n_skipped"] == n
    want = check_dense(ctx, R.INT, np.zeros(0, np.int32), K.REF_RANGE)     # an empty block initialises and reads nothing
    assert want[1]["n_cells"] == 0 and want[1]["min_at"] == -1 and (want[0] == 0).all()


def test_dense_the_two_zeroes(ctx):
    a, b = K.zero_blocks()
    trip = K.first_trip(R.FLOAT)
    for pad in (0, 3, trip, 2 * trip + 1):                                  # the zeroes in one lane's load, in two lanes, in two workgroups
        for z in (a, b):
            v = np.concatenate([np.full(pad, 4.0, np.float32), z[:4], np.full(pad, 9.0, np.float32), z[4:]])
            want = check_dense(ctx, R.FLOAT, v, K.REF_RANGE)
            assert want[1]["min_at"] == pad + 1 and R.bits(want[1]["min"]) == R.bits(float(z[1]))
    want = check_dense(ctx, R.FLOAT, -a, K.REF_RANGE)                       # and for a maximum of zero
    assert want[1]["max_at"] == 1 and R.bits(want[1]["max"]) == R.bits(0.0)


@pytest.mark.parametrize("elem_type", TYPES, ids=TYPE_IDS)
def test_dense_ties_across_lanes_waves_and_workgroups(ctx, elem_type):
    """the same extreme in two different lanes, waves and workgroups' parts: the smaller index wins, whichever part holds it"""
    rng = np.random.default_rng(700 + elem_type)
    trip, per = K.first_trip(elem_type), K.cells_per_load(elem_type)
    n = 4 * trip
    for lo_at, hi_at in (((trip + 100, 2 * trip + 3), (2 * trip + 50, 9)), ((5, 5 + per), (64 * per + 1, 3 * 64 * per)),
                         ((3 * trip + 1, 3 * trip + 2), (0, n - 1)), ((n - 1, 2), (trip - 1, trip))):
        v = K.dem_like(rng, n, elem_type, -300, 500)
        v[list(lo_at)], v[list(hi_at)] = -700, 900
        want = check_dense(ctx, elem_type, v, (-300, 500, 1.0), first_cell=10 ** 12)
        assert want[1]["min_at"] == 10 ** 12 + min(lo_at) and want[1]["max_at"] == 10 ** 12 + min(hi_at)
        assert want[1]["min"] == -700 and want[1]["max"] == 900


def test_dense_sums_leave_int32(ctx):
    v = np.full(5000, 2 ** 31 - 7, np.int32)
    v[::3] = 2 ** 31 - 9
    want = check_dense(ctx, R.INT, v, (2 ** 31 - 20, 2 ** 31 - 1, 1.0))
    assert want[1]["sum_i"] > 2 ** 40 and want[1]["sum_samples"] == want[1]["sum_i"] and want[1]["n_samples"] == 5000
    want = check_dense(ctx, R.INT, -v, (-2 ** 31 + 1, -2 ** 31 + 20, 1.0))
    assert want[1]["sum_i"] < -2 ** 40 and want[1]["sum_samples"] == want[1]["sum_i"] + 5000


# ---------------------------------------------------------------- dense form: strips; the host form

@pytest.mark.parametrize("elem_type", TYPES, ids=TYPE_IDS)
def test_dense_accumulates_strips(ctx, elem_type):
    """three strips with GF_TAB_ACCUMULATE and first_cell against one call over the whole, a tie of the extremes across the strips;
    in both tables' forms (LDS and global atomics)"""
    rng = np.random.default_rng(800 + elem_type)
    n = 3 * K.first_trip(elem_type) + 10
    cuts = [0, K.first_trip(elem_type) + 6, 2 * K.first_trip(elem_type) - 2, n]
    v = K.dem_like(rng, n, elem_type, -300, 500)
    v[[cuts[1] - 1, cuts[1], cuts[2] + 9]] = -700
    v[[cuts[2] + 1, 7, cuts[1] + 1]] = 900
    strips = list(zip(cuts[:-1], cuts[1:]))
    for window in ((-300, 500, 1.0), (-300, K.LDS_MAX_BINS + 500, 1.0)):
        whole = R.dense(v, elem_type, *window, first_cell=1000)
        for order in (strips, strips[::-1]):
            got = dense_dev(ctx, elem_type, v, window, strips=order, first_cell=1000)
            assert np.array_equal(got[0], whole[0]) and R.same_summary(got[1], whole[1]), (elem_type, window, order, got[1], whole[1])
        assert whole[1]["min_at"] == 1000 + cuts[1] - 1 and whole[1]["max_at"] == 1007 and whole[1]["n_cells"] == n


@pytest.mark.parametrize("elem_type", TYPES, ids=TYPE_IDS)
def test_dense_host_form_equals_the_device_form(ctx, elem_type):
    rng = np.random.default_rng(900 + elem_type)
    v = K.dem_like(rng, 2 * K.first_trip(elem_type) + 9, elem_type)
    dev = dense_dev(ctx, elem_type, v, K.REF_RANGE, fill_i=-5, skip_fill=True, first_cell=40)
    host = ctx.tabulate_dense(NAMES[elem_type], v, *K.REF_RANGE, fill_i=-5, skip_fill=True, first_cell=40)
    assert np.array_equal(host[0], dev[0]) and R.same_summary(host[1], dev[1])
    half = v.size // 2 & ~1
    acc = ctx.tabulate_dense(NAMES[elem_type], v[:half], *K.REF_RANGE, fill_i=-5, skip_fill=True, first_cell=40)
    acc = ctx.tabulate_dense(NAMES[elem_type], v[half:], *K.REF_RANGE, fill_i=-5, skip_fill=True, first_cell=40 + half, into=acc)
    assert np.array_equal(acc[0], dev[0]) and R.same_summary(acc[1], dev[1])
    empty = ctx.tabulate_dense(NAMES[elem_type], v[:0], 0, 9, 1.0)
    assert (empty[0] == 0).all() and empty[0].size == 11 and R.same_summary(empty[1], R.empty_summary())


# ---------------------------------------------------------------- symbol form

@pytest.mark.parametrize("elem_type", TYPES, ids=TYPE_IDS)
def test_symbols_sizes(ctx, elem_type):
    """1, 63, 64, 65 cells, one scatter workgroup's share - 1, itself and + 1, three workgroups and a few more"""
    rng = np.random.default_rng(1000 + elem_type)
    share = K.sort_share(1000)
    assert share == K.SORT_THREADS
    sizes = [1, 63, 64, 65, share - 1, share, share + 1, 3 * share + 5, 9 * share - 1]
    whole = K.dem_like(rng, sizes[-1], elem_type, -200, 300)
    for n in sizes:
        _, _, s = check_symbols(ctx, elem_type, whole[:n])
        assert s["n_samples"] == n
    assert s["n_unique"] > 0 and s["n_repeated"] > 0 and s["max_count"] > 1


def test_symbols_digits(ctx):
    """all keys equal; keys that differ in one byte only (each of the four); all 256 values of every digit; 0 and 0xFFFFFFFF; every
    key distinct; a count that needs more than 16 bits"""
    rng = np.random.default_rng(11)
    n = 5 * K.SORT_THREADS + 77
    for key in (0, 0xFFFFFFFF, 0x80000000, 0x12345678):
        sym, cnt, s = check_symbols(ctx, R.INT, np.full(n, key, np.uint32).view(np.int32))
        assert sym.tolist() == [key] and cnt.tolist() == [n] and (s["n_unique"], s["n_repeated"], s["max_count"]) == (0, 1, n)
    for byte in range(4):
        keys = (rng.permutation(np.arange(n, dtype=np.uint32) % np.uint32(256)) << np.uint32(8 * byte)) | np.uint32(0x5A5A5A5A & ~(0xFF << 8 * byte))
        sym, _, s = check_symbols(ctx, R.INT, keys.view(np.int32))
        assert s["n_symbols"] == 256 == np.unique(sym >> np.uint32(8 * byte) & np.uint32(255)).size
    every = rng.permutation(np.repeat(np.arange(256, dtype=np.uint32) * np.uint32(0x01010101), 5))
    _, cnt, s = check_symbols(ctx, R.INT, every.view(np.int32))
    assert s["n_symbols"] == 256 and (cnt == 5).all()
    both = rng.permutation(np.repeat(np.array([0, 0xFFFFFFFF], np.uint32), [300, 301]))
    sym, cnt, _ = check_symbols(ctx, R.INT, both.view(np.int32))
    assert sym.tolist() == [0, 0xFFFFFFFF] and cnt.tolist() == [300, 301]
    distinct = rng.permutation((np.arange(20000, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(2 ** 32)).astype(np.uint32))
    _, _, s = check_symbols(ctx, R.INT, distinct.view(np.int32))
    assert s["n_unique"] == s["n_symbols"] == 20000 and s["n_repeated"] == 0 and s["max_count"] == 1
    wide = np.concatenate([np.full(70000, -5, np.int32), distinct[:100].view(np.int32)])
    _, _, s = check_symbols(ctx, R.INT, rng.permutation(wide))
    assert s["max_count"] == 70000 > 65535


def test_symbols_floats_and_shorts(ctx):
    z = np.tile(np.array([0.0, -0.0, np.nan, 1.0, -1.0, 0.0], np.float32), 100)
    z.view(np.uint32)[2::12] = 0x7FC00001                                  # another NaN payload
    z.view(np.uint32)[8] = 0xFFC00000                                      # a negative NaN, once
    sym, cnt, s = check_symbols(ctx, R.FLOAT, z)
    assert sym.tolist() == [0, 0x3F800000, 0x7FC00000, 0x7FC00001, 0x80000000, 0xBF800000, 0xFFC00000]
    assert cnt.tolist() == [200, 100, 49, 50, 100, 100, 1] and s["n_unique"] == 1
    v = np.tile(np.array([5, -1, 0, -32768, 32767, -1, 7], np.int16), 90)[:-1]        # an odd count
    sym, cnt, s = check_symbols(ctx, R.SHORT, v)
    assert sym.tolist() == [0, 5, 7, 32767, 0xFFFF8000, 0xFFFFFFFF] and cnt.tolist() == [90, 90, 89, 90, 90, 180]


@pytest.mark.parametrize("elem_type", [R.INT, R.FLOAT], ids=["int", "float"])
def test_symbols_table_capacity(ctx, elem_type):
    """a table of 0 entries (NULL tables: the scalars alone), of n_symbols - 1, n_symbols and n_symbols + 1: n_written, the complete
    scalars, and nothing written behind n_written; the host form reports the table that is too small"""
    from gridfour_amd import _lib
    v = (((K.int_stream(7 * K.SORT_THREADS + 3, 1200 + elem_type) >> np.uint32(7)) % np.uint32(120)).astype(np.int32) - 60).astype(R.DTYPES[elem_type])
    v = v * np.float32(0.5) if elem_type == R.FLOAT else v
    n_sym = R.symbols(v, elem_type)[2]["n_symbols"]
    assert n_sym > 50
    for cap in (0, 1, n_sym - 1, n_sym, n_sym + 1):
        _, _, s = check_symbols(ctx, elem_type, v, cap=cap)
        assert s["n_written"] == min(cap, n_sym) and s["n_symbols"] == n_sym
    want_sym, want_cnt, want = R.symbols(v, elem_type)
    for cap in (0, n_sym - 1, n_sym, n_sym + 1, None):
        sym, cnt, s = ctx.tabulate_symbols(NAMES[elem_type], v, table_cap=cap)
        n = n_sym if cap is None else min(cap, n_sym)
        assert s == dict(want, n_written=n) and np.array_equal(sym, want_sym[:n]) and np.array_equal(cnt, want_cnt[:n]), cap
    from gridfour_amd.codec import TAB_SYMBOLS
    table, s = np.zeros(4, np.uint32), np.zeros(1, TAB_SYMBOLS)
    vv = np.ascontiguousarray(v)
    st = _lib.lib().gf_block_tabulate_symbols(ctx.handle, elem_type, C.c_void_p(vv.ctypes.data), vv.size, C.c_void_p(table.ctypes.data),
                                               C.c_void_p(table.ctypes.data), 1, C.c_void_p(s.ctypes.data))
    assert st == _lib.ERR_CAPACITY and s["n_written"][0] == 1 and s["n_symbols"][0] == n_sym
    empty = ctx.tabulate_symbols(NAMES[elem_type], v[:0])
    assert empty[0].size == 0 and all(x == 0 for x in empty[2].values())


def test_symbols_beyond_one_block_of_the_scan(ctx):
    """enough sort workgroups for the histogram's scan to need more than one trip of its middle phase (more sums than its workgroup
    has lanes), with keys spread over all four digits"""
    n = 300000
    n_wg = -(-n // K.sort_share(n))
    assert n_wg * 256 > K.SCAN_BLOCK * K.SORT_THREADS and n_wg > 3
    keys = K.int_stream(n)
    keys[::3] &= np.uint32(0x000F00FF)                                     # repeats among them
    _, _, s = check_symbols(ctx, R.INT, keys.view(np.int32))
    assert s["n_unique"] > 1000 and s["n_repeated"] > 1000
    f = (keys >> np.uint32(12)).astype(np.float32) * np.float32(0.125) - np.float32(9000.0)
    check_symbols(ctx, R.FLOAT, f)
    check_symbols(ctx, R.SHORT, (keys >> np.uint32(16)).astype(np.uint16).view(np.int16))


def _share_sizes(share):
    """cell counts that give a sort workgroup `share` keys: a whole number of shares - 1 and + 1, and a last workgroup whose share
    ends in the middle of a round"""
    k = {2 * K.SORT_THREADS: 1100, K.SHARE_MAX: K.SPREAD - 120}[share]
    sizes = [k * share - 1, k * share + 1, k * share + share - K.SORT_THREADS - 45]
    assert all(K.sort_share(n) == share for n in sizes) and share // K.SORT_THREADS >= 2
    return sizes


@pytest.mark.parametrize("share", [2 * K.SORT_THREADS, K.SHARE_MAX], ids=["two_rounds", "share_max"])
def test_symbols_shares_of_several_rounds(ctx, share):
    """blocks large enough for a sort workgroup to own more than one round of keys (two rounds; GF_TAB_SORT_SHARE_MAX / 256 of
    them): the running offsets carried from round to round, the wave counts cleared between rounds, the histogram's several trips,
    and a last share that ends in the middle of a round -- keys spread over all four digits, every table entry against the model"""
    for j, n in enumerate(_share_sizes(share)):
        keys = K.int_stream(n, seed=31 + j)
        keys[::2] &= np.uint32(0x000F00FF)                                 # repeats; the other half mostly distinct
        keys[5::7] |= np.uint32(0x80000000)
        _, cnt, s = check_symbols(ctx, R.INT, keys.view(np.int32))
        assert s["n_samples"] == n and s["n_unique"] > 1000 and s["max_count"] > 2
    f = (keys >> np.uint32(9)).astype(np.float32) * np.float32(0.25) - np.float32(1e6)      # the last size once more as FLOAT and SHORT
    check_symbols(ctx, R.FLOAT, f)
    check_symbols(ctx, R.SHORT, (keys >> np.uint32(11)).astype(np.uint16).view(np.int16))


# ---------------------------------------------------------------- composed: a block read from tile records, tabulated in place

def test_block_read_then_tabulated_in_place(master5, records4):
    """the three elements of tests/test_gpu_blocks.py's records (short; int-coded float, delivered as float; float) read into
    device memory by gf_block_read_elems_dev and tabulated where they lie, against the model on the model's block"""
    import gridfour_amd
    from gridfour_amd._lib import check, lib
    from gridfour_amd.codec import TAB_SUMMARY, TAB_SYMBOLS
    r, ctx = records4, master5.ctx
    rect = (13, 27, 80, 150)
    n = rect[2] * rect[3]
    model = TB._model4(r, rect)                                            # per element the block's bits
    specs, dtypes = master5._elem_specs(RE.ELEMS3)
    master5._fill_specs(specs, RE.ELEMS3, TB.FILLS4)
    blob, offsets = np.ascontiguousarray(r["blob"], np.uint8), np.ascontiguousarray(r["offsets"], np.uint64)
    nt, ne = offsets.size - 1, 3
    grid, rc = np.array(TB.GRID4 + TB.TILE4, np.int32), np.array(rect, np.int32)
    d_blob = gridfour_amd.DeviceBuffer(ctx, blob.size + 32).fill(0).upload(blob)
    d_off = gridfour_amd.DeviceBuffer(ctx, offsets.nbytes).upload(offsets)
    d_blk = [gridfour_amd.DeviceBuffer(ctx, n * np.dtype(dt).itemsize + 16).fill(0) for dt in dtypes]
    d_st = gridfour_amd.DeviceBuffer(ctx, ne * nt * 4 + 16).fill(0)
    outs = []
    try:
        ptrs = (C.c_void_p * ne)(*[b.ptr.value for b in d_blk])
        cod = master5._codecs_arg()
        check(lib().gf_block_read_elems_dev(ctx.handle, None, C.c_void_p(cod.ctypes.data), master5.codecs.size, C.c_void_p(specs.ctypes.data), ne,
                                            C.c_void_p(grid.ctypes.data), C.c_void_p(rc.ctypes.data), nt, d_blob.ptr, blob.size, d_off.ptr, 1, ptrs,
                                            d_st.ptr), "gf_block_read_elems_dev")
        for e, elem_type in enumerate((R.SHORT, R.FLOAT, R.FLOAT)):
            want_block = model[e].view(R.DTYPES[elem_type]).ravel()
            window = (-200, 1200, 1.0) if elem_type == R.SHORT else (-50, 400, 4.0)
            fill = TB.FILLS4[0] if e == 0 else 0
            dense_want = R.dense(want_block, elem_type, *window, fill_i=fill, skip_fill=True)
            sym_want = R.symbols(want_block, elem_type)
            cnt, summ = Guarded(ctx, dense_want[0].size * 4), Guarded(ctx, TAB_SUMMARY.itemsize)
            sym, scn, ssum = Guarded(ctx, n * 4), Guarded(ctx, n * 4), Guarded(ctx, TAB_SYMBOLS.itemsize)
            outs += [cnt, summ, sym, scn, ssum]
            ctx.tabulate_dense_dev(elem_type, d_blk[e].ptr, n, *window, cnt.ptr, summ.ptr, fill_i=fill, skip_fill=True)
            ctx.tabulate_symbols_dev(elem_type, d_blk[e].ptr, n, sym.ptr, scn.ptr, n, ssum.ptr)
            ctx.synchronize()
            assert np.array_equal(d_blk[e].download(np.uint8, want_block.nbytes), want_block.view(np.uint8)), e      # the block is the model's, still
            assert np.array_equal(cnt.get(np.int32), dense_want[0]) and R.same_summary(K.summary_dict(summ.get(TAB_SUMMARY)), dense_want[1]), e
            s = ssum.get(TAB_SYMBOLS)
            assert {k: s[k][0].item() for k in TAB_SYMBOLS.names} == sym_want[2], e
            k = sym_want[2]["n_symbols"]
            assert np.array_equal(sym.get(np.uint32)[:k], sym_want[0]) and np.array_equal(scn.get(np.int32)[:k], sym_want[1]), e
            assert dense_want[1]["n_samples"] > 0 and dense_want[1]["n_skipped"] > 0 and k > 10, e
    finally:
        for b in [d_blob, d_off, d_st] + d_blk + outs:
            b.free()
