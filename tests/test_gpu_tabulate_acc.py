"""Symbol tables merged and strips accumulated on the GPU (gf_tab_symbols_merge[_dev], gf_block_tabulate_symbols_acc[_dev],
gf_block_read_tabulated_symbols_elems[_dev]): every table entry and every scalar against the numpy model of
tests/tabulate_acc_ref.py, at the smallest shapes at which the kernels can still go wrong.  The sizes come from the
implementation's constants, read out of gvrs_tabulate_common.h by tests/tabulate_acc_cases.py.  Guard bands of 0xA5 bytes stand on
both sides of every output, the outputs themselves are pre-filled with 0xA5, and the inputs are read back unchanged.  Totals past
2^31 - 1 cells are reached through hand-built summaries alone."""
import ctypes as C

import numpy as np
import pytest

import tabulate_acc_cases as KA
import tabulate_acc_ref as A
import tabulate_cases as K
import tabulate_ref as R
from test_gpu_records_dev import ctx      # noqa: F401  (fixture)
from test_gpu_tabulate import Block, Guarded, symbols_dev

pytestmark = pytest.mark.gpu
B, P = KA.MERGE_BLOCK, KA.MERGE_PER
NAMES = {R.INT: "int", R.SHORT: "short", R.FLOAT: "float"}


def _summary(a):
    from gridfour_amd.codec import TAB_SYMBOLS
    return {k: a[k][0].item() for k in TAB_SYMBOLS.names}


class DevTable:
    """a table in device memory, its arrays of exactly `cap` entries (None: its own length)"""

    def __init__(self, ctx, t, cap=None):
        from gridfour_amd.codec import TAB_SYMBOLS
        self.t, self.cap = t, t[0].size if cap is None else cap
        s = np.zeros(1, TAB_SYMBOLS)
        for k in TAB_SYMBOLS.names:
            s[k] = t[2][k]
        self.parts = [Block(ctx, np.ascontiguousarray(t[0][:self.cap], np.uint32)), Block(ctx, np.ascontiguousarray(t[1][:self.cap], np.int32)),
                      Block(ctx, s.view(np.uint8))]

    def args(self):
        return (self.parts[0].ptr() if self.cap else None, self.parts[1].ptr() if self.cap else None, self.parts[2].ptr(), self.cap)

    def unchanged(self):
        return all(p.unchanged() for p in self.parts)

    def free(self):
        for p in self.parts:
            p.free()


class OutTable:
    def __init__(self, ctx, cap):
        from gridfour_amd.codec import TAB_SYMBOLS
        self.cap = cap
        self.sym, self.cnt, self.sum = Guarded(ctx, cap * 4), Guarded(ctx, cap * 4), Guarded(ctx, TAB_SYMBOLS.itemsize)

    def args(self):
        return (self.sym.ptr if self.cap else None, self.cnt.ptr if self.cap else None, self.cap, self.sum.ptr)

    def as_input(self):
        return (self.sym.ptr if self.cap else None, self.cnt.ptr if self.cap else None, self.sum.ptr, self.cap)

    def get(self):
        """(the table as written, whole arrays) -- also checks the guard bands and that nothing stands behind n_written"""
        from gridfour_amd.codec import TAB_SYMBOLS
        sym, cnt, s = self.sym.get(np.uint32), self.cnt.get(np.int32), _summary(self.sum.get(TAB_SYMBOLS))
        n = s["n_written"]
        assert 0 <= n <= self.cap and (sym[n:] == 0xA5A5A5A5).all() and (cnt[n:].view(np.uint32) == 0xA5A5A5A5).all(), "table written behind n_written"
        return sym[:n], cnt[:n], s

    def guards(self):
        for x in (self.sym, self.cnt, self.sum):
            x.get(np.uint8)

    def free(self):
        for x in (self.sym, self.cnt, self.sum):
            x.free()


def check_merge(ctx, a, b, cap=None, cap_a=None, cap_b=None):
    want = A.merge(a, b, cap_a, cap_b)
    cap = want[0].size + 3 if cap is None else cap
    da, db, out = DevTable(ctx, a, cap_a), DevTable(ctx, b, cap_b), OutTable(ctx, cap)
    try:
        ctx.tab_symbols_merge_dev(*da.args(), *db.args(), *out.args())
        ctx.synchronize()
        assert da.unchanged() and db.unchanged(), "input table changed"
        got = out.get()
        assert A.same(got, A.cut(want, cap)), (a[0].size, b[0].size, cap, got[2], want[2])
        return want
    finally:
        for x in (da, db, out):
            x.free()


# ---------------------------------------------------------------- the merge

def test_merge_empty_and_overlap_shapes(ctx):
    rng = np.random.default_rng(31)
    lo, hi = KA.random_table(rng, 700, 3000), KA.random_table(rng, 900, 3000)
    far = A.table(hi[0] + np.uint32(2 ** 31), hi[1])
    evens, odds = A.table(np.arange(0, 1600, 2), np.arange(800) % 7 + 1), A.table(np.arange(1, 1601, 2), np.arange(800) % 5 + 1)
    gap = A.table(np.concatenate([lo[0], lo[0] + np.uint32(2 ** 30)]), np.concatenate([lo[1], lo[1]]))
    inside = A.table(hi[0] + np.uint32(2 ** 20), hi[1])
    for a, b in ((A.EMPTY, A.EMPTY), (lo, A.EMPTY), (A.EMPTY, lo), (lo, far), (far, lo), (lo, lo), (evens, odds), (odds, evens), (gap, inside),
                 (inside, gap), (lo, hi)):
        want = check_merge(ctx, a, b)
        assert want[2]["n_samples"] == a[2]["n_samples"] + b[2]["n_samples"] and want[2]["reserved"] == 0
    assert check_merge(ctx, lo, lo)[2]["n_symbols"] == 700 and check_merge(ctx, evens, odds)[2]["n_symbols"] == 1600


def test_merge_chunk_sizes(ctx):
    """merged sequences of one chunk - 1, one chunk, one chunk + 1 and three chunks + 1 positions, split between the tables in
    three ways, with many equal pairs"""
    rng = np.random.default_rng(32)
    for total in (B - 1, B, B + 1, 3 * B + 1):
        for na in (total // 2, 1, total - 3):
            a, b = KA.random_table(rng, na, 2 * total, wrap=True), KA.random_table(rng, total - na, 2 * total, wrap=True)
            check_merge(ctx, a, b)


def test_merge_an_equal_pair_at_every_seam(ctx):
    """three chunks; one symbol in both tables, its pair of neighbours ending in front of a seam, cut by it and starting behind it
    -- at the seams between chunks and at a seam between two lanes; the long table as A and as B, and with interleaved tables"""
    n = 3 * B - 1
    long = A.table(np.arange(n) * 4, np.arange(n) % 9 + 1)
    for seam in (B, 2 * B, P, B + 3 * P):
        for q in (seam - 2, seam - 1, seam):                               # the pair stands at positions q, q + 1
            one = A.table([4 * q], [100])
            for a, b in ((long, one), (one, long)):
                want = check_merge(ctx, a, b)
                assert want[0].size == n and want[1][q] == q % 9 + 101
    m = 3 * B // 2
    evens, odds = np.arange(m) * 2, np.arange(m) * 2 + 1                   # position p of the merged sequence holds p ...
    for seam in (B, 2 * B):
        for q in (seam - 2, seam - 1, seam):                               # ... but for q, which both tables hold: positions q, q + 1
            sa, sb = np.union1d(evens, [q]), np.union1d(odds, [q])
            want = check_merge(ctx, A.table(sa, np.full(sa.size, 5)), A.table(sb, np.ones(sb.size)))
            assert want[0].size == 2 * m and want[1][q] == 6 and set(np.delete(want[1], q).tolist()) == {1, 5}


def test_merge_corner_symbols_wraps_caps_and_flags(ctx):
    a = A.table(KA.CORNERS, [2 ** 31 - 1, -1, -2 ** 31, 7])
    b = A.table(KA.CORNERS, [1, 1, -2 ** 31, 2 ** 31 - 7])
    want = check_merge(ctx, a, b)
    assert want[0].tolist() == list(KA.CORNERS) and want[1].tolist() == [-2 ** 31, 0, 0, -2 ** 31]
    assert (want[2]["n_symbols"], want[2]["n_unique"], want[2]["n_repeated"], want[2]["max_count"]) == (4, 0, 0, 0)
    for keep in ([0, 3], [1, 2], [0], [3]):
        check_merge(ctx, a, A.table(np.array(KA.CORNERS)[keep], b[1][keep]))
    # n_samples past 2^32 and past 2^31 - 1 cells, by hand-built summaries
    big = check_merge(ctx, A.table([1, 2], [5, 6], n_samples=2 ** 32 + 11), A.table([2, 3], [2 ** 31 - 1, 1], n_samples=2 ** 33))
    assert big[2]["n_samples"] == 2 ** 32 + 11 + 2 ** 33 and big[1].tolist() == [5, -2 ** 31 + 5, 1]
    # the out table's capacity
    rng = np.random.default_rng(33)
    x, y = KA.random_table(rng, B + 40, 2 * B), KA.random_table(rng, B - 9, 2 * B)
    n_out = A.merge(x, y)[0].size
    for cap in (n_out, n_out - 1, 1, 0):
        want = check_merge(ctx, x, y, cap=cap)
        assert want[2]["n_symbols"] == n_out
    # a truncated input: the flag, sticky through a second merge on either side; a cap above and below the summary's n_written
    cut = A.table(x[0][:B], x[1][:B], n_samples=x[2]["n_samples"], n_symbols=x[0].size)
    flagged = check_merge(ctx, cut, y)
    assert flagged[2]["reserved"] == A.TRUNCATED
    assert check_merge(ctx, flagged, x)[2]["reserved"] == A.TRUNCATED and check_merge(ctx, x, flagged)[2]["reserved"] == A.TRUNCATED
    roomy = check_merge(ctx, x, y, cap_a=x[0].size, cap_b=y[0].size)
    assert roomy[2]["reserved"] == 0
    padded = (np.append(x[0], [7, 7, 7]).astype(np.uint32), np.append(x[1], [9, 9, 9]).astype(np.int32), x[2])     # cap_a > n_written: the rest is not read as entries
    assert A.same(check_merge(ctx, padded, y, cap_a=x[0].size + 3), roomy)
    short = check_merge(ctx, x, y, cap_a=B - 5)                            # cap_a < n_written: the entries it has, and the flag
    assert short[2]["reserved"] == A.TRUNCATED and short[0].size < n_out


# ---------------------------------------------------------------- a strip onto a table

def acc_dev(ctx, elem_type, values, cuts, cap=None, first=0):
    """the strips values[cuts[k]:cuts[k + 1]] counted one after another onto a table that starts empty, the two tables taking
    turns; first: cells in front of the block (a SHORT block at an odd cell)"""
    v = np.ascontiguousarray(values, R.DTYPES[elem_type]).ravel()
    cap = v.size if cap is None else cap
    blk = Block(ctx, np.concatenate([np.zeros(first, v.dtype), v]))
    tables = [OutTable(ctx, cap), OutTable(ctx, cap)]
    try:
        into = (None, None, None, 0)
        for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            out = tables[k & 1]
            ctx.tabulate_symbols_acc_dev(elem_type, blk.ptr(first + a), b - a, *into, *out.args())
            into = out.as_input()
        ctx.synchronize()
        assert blk.unchanged(), "input block changed"
        last = (len(cuts) - 2) & 1
        tables[last ^ 1].guards()
        return tables[last].get()
    finally:
        for x in [blk] + tables:
            x.free()


def check_short(ctx, v, first=0):
    want = R.symbols(v, R.SHORT)
    got = acc_dev(ctx, R.SHORT, v, [0, v.size], cap=min(v.size, 65536) + 2, first=first)
    assert A.same(got, want), (v.size, first, got[2], want[2])
    return want


def test_short_counters_sizes_and_alignment(ctx):
    rng = np.random.default_rng(41)
    trip = 8 * K.THREADS
    grid = KA.SHORT_MAX_GROUPS * trip
    whole = K.dem_like(rng, grid + 1, R.SHORT, KA.WIN_LO - 300, KA.WIN_HI + 300)
    for n in (1, 7, trip - 1, trip + 1, grid + 1):
        check_short(ctx, whole[:n])
    for first in (1, 3, 7):                                                # a block that starts at an odd cell
        for n in (1, 6, 9, trip + 2):
            check_short(ctx, whole[100:100 + n], first=first)


def test_short_counters_values(ctx):
    edges = np.array([-32768, 32767, KA.WIN_LO - 1, KA.WIN_LO, KA.WIN_LO + 1, KA.WIN_HI - 1, KA.WIN_HI, KA.WIN_HI + 1, 0, -1], np.int16)
    want = check_short(ctx, np.repeat(edges, np.arange(1, 11)))
    assert want[0].tolist() == A.short_order(edges).tolist() and want[2]["n_unique"] == 1
    for value in (5, KA.WIN_HI + 1, -32768):                               # one counter under contention, in the window and outside it
        want = check_short(ctx, np.full(2 ** 20, value, np.int16))
        assert want[1].tolist() == [2 ** 20] and want[2]["max_count"] == 2 ** 20
    ramp = np.random.default_rng(42).permutation(np.arange(-32768, 32768)).astype(np.int16)
    want = check_short(ctx, ramp)
    assert want[2]["n_unique"] == 65536 and np.array_equal(want[0] & np.uint32(0xFFFF), np.arange(65536, dtype=np.uint32))


@pytest.mark.parametrize("elem_type", [R.INT, R.SHORT, R.FLOAT], ids=["int", "short", "float"])
def test_accumulate_strips(ctx, elem_type):
    """about 0.6 M cells as 1, 2, 5 and 37 unequal strips with an empty and a one-cell strip among them: the model's table whatever
    the split, which is also what the one-call form gives"""
    rng = np.random.default_rng(50 + elem_type)
    n = 600011
    v = K.dem_like(rng, n, elem_type)
    if elem_type == R.FLOAT:
        v[:6] = np.array([0.0, -0.0, np.nan, np.nan, -0.0, 1.5], np.float32)
        v.view(np.uint32)[3] = 0x7FC00001                                  # another NaN payload
        v[n - 6:] = v[:6]
    whole = R.symbols(v, elem_type)
    one_sym, one_cnt, one_s = symbols_dev(ctx, elem_type, v, whole[0].size)
    assert A.same((one_sym, one_cnt, one_s), whole)                        # (the unchanged one-call form, as a cross-check)
    for k in (1, 2, 5, 37):
        at = np.sort(rng.choice(np.arange(1, n), k - 1, replace=False)).tolist() if k > 1 else []
        cuts = [0] + at + [n]
        if k >= 5:
            assert cuts[2] > cuts[1] + 1
            cuts = cuts[:2] + [cuts[1], cuts[1] + 1] + cuts[2:]            # an empty strip, then a strip of one cell
        strips = [v[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        want = A.accumulate(strips, elem_type)
        assert A.same(want, whole)
        got = acc_dev(ctx, elem_type, v, cuts, cap=whole[0].size + 1)
        assert A.same(got, want), (elem_type, k, got[2], want[2])
    if elem_type == R.FLOAT:
        assert {0, 0x80000000, 0x7FC00000, 0x7FC00001} <= set(whole[0].tolist())


def test_accumulate_onto_hand_built_tables(ctx):
    """an in-table whose counts wrap and whose n_samples lies past 2^32; an in-table without samples is empty; no cells: the
    in-table copied through; a table too small"""
    v = np.array([5, 9, 9, 12, 5], np.int32)
    start = A.table([5, 9, 11], [2 ** 31 - 1, -2, 3], n_samples=2 ** 32 + 4)
    want = A.accumulate([v], R.INT, into=start)
    assert want[1].tolist() == [-2 ** 31 + 1, 0, 3, 1] and want[2]["n_samples"] == 2 ** 32 + 9
    for values, into, cap in ((v, start, 6), (v[:0], start, 6), (v, A.table([5, 9], [1, 1], n_samples=0), 6), (v, start, 2), (v[:0], start, 0)):
        want = A.accumulate([values], R.INT, into=into)
        din, blk, out = DevTable(ctx, into), Block(ctx, values if values.size else np.zeros(1, np.int32)), OutTable(ctx, cap)
        try:
            ctx.tabulate_symbols_acc_dev(R.INT, blk.ptr(), values.size, *din.args(), *out.args())
            ctx.synchronize()
            assert din.unchanged() and A.same(out.get(), A.cut(want, cap)), (values.size, cap)
        finally:
            for x in (din, blk, out):
                x.free()


def test_host_forms(ctx):
    from gridfour_amd import _lib
    rng = np.random.default_rng(61)
    x, y = KA.random_table(rng, B + 40, 2 * B, wrap=True), KA.random_table(rng, 2 * B - 9, 2 * B)
    want = A.merge(x, y)
    assert A.same(ctx.tab_symbols_merge(x, y), want)
    assert A.same(ctx.tab_symbols_merge(x, y, table_cap=10), A.cut(want, 10))
    cut = A.table(x[0][:B], x[1][:B], n_samples=x[2]["n_samples"], n_symbols=x[0].size)
    assert ctx.tab_symbols_merge(cut, y)[2]["reserved"] == A.TRUNCATED
    for elem_type in (R.INT, R.SHORT, R.FLOAT):
        v = K.dem_like(rng, 20001, elem_type)
        t = None
        for a, b in ((0, 9000), (9000, 9001), (9001, 9001), (9001, 20001)):
            t = ctx.tabulate_symbols_acc(NAMES[elem_type], v[a:b], into=t)
        assert A.same(t, R.symbols(v, elem_type)), elem_type
    small = ctx.tabulate_symbols_acc("int", np.arange(50, dtype=np.int32), table_cap=7)
    assert small[0].tolist() == list(range(7)) and small[2]["n_symbols"] == 50 and small[2]["n_written"] == 7
    from gridfour_amd.codec import TAB_SYMBOLS
    vv, table, s = np.arange(50, dtype=np.int32), np.zeros(8, np.uint32), np.zeros(1, TAB_SYMBOLS)
    p = lambda a: C.c_void_p(a.ctypes.data)
    st = _lib.lib().gf_block_tabulate_symbols_acc(ctx.handle, 0, p(vv), 50, None, None, None, 0, p(table), p(table[4:]), 4, p(s))
    assert st == _lib.ERR_CAPACITY and s["n_written"][0] == 4 and s["n_symbols"][0] == 50


# ---------------------------------------------------------------- composed: rectangles read from tile records onto a table

def test_rectangles_read_from_records_and_tabulated(ctx):
    """a 50 x 70 raster of an INT and an int-coded-float element, written as 3 x 3 tile records by the record writer and read back
    as two rectangles: the table of the INT cells, and the table of the ICF element's codes"""
    rng = np.random.default_rng(71)
    tile, grid = (20, 30), (50, 70)
    ints = K.dem_like(rng, grid[0] * grid[1], R.INT, -300, 500).reshape(grid)
    codes = K.dem_like(rng, grid[0] * grid[1], R.INT, -900, 900).reshape(grid)
    icf = ("icf", 4.0, 0.0, -2 ** 31, np.float32(np.nan))
    elems = ["int", icf]
    blocks = [ints, (codes / 4.0).astype(np.float32)]                      # (a code / 4 is exact in a float)
    import gridfour_amd
    import test_gpu_block_write as TW
    master = gridfour_amd.CodecMasterHip(codec_list=[TW.HUFFMAN, TW.CANON], context=ctx)
    idx, records, used, status = master.write_block_dev(tile[0], tile[1], grid, (0, 0) + grid, blocks, elems)
    assert (status == 0).all() and len(records) == 9
    blob, offsets = TW._blob(records)
    back, st = master.read_block_downsampled_dev(tile[0], tile[1], grid, (0, 0) + grid, 1, blob, offsets, elems)
    assert (st == 0).all() and np.array_equal(back[0], ints) and np.array_equal(back[1], codes)      # the ICF element as its codes
    rects = ((0, 0, 23, 70), (23, 0, 27, 70))
    for which, model in ((0, ints), (1, codes)):
        want = A.accumulate([model[r0:r0 + nr, c0:c0 + nc] for r0, c0, nr, nc in rects], R.INT)
        for read in (master.read_block_tabulated_symbols_dev, master.read_block_tabulated_symbols):
            t = None
            for rect in rects:
                t, st = read(tile[0], tile[1], grid, rect, blob, offsets, elems, which, into=t)
                assert (st == 0).all()
            assert A.same(t, want) and A.same(t, R.symbols(model, R.INT)), which
