"""The LSOP08 kernels (gvrs_lsop8.hip) at the shapes where their indexing changes, bit for bit against tests/lsop08_ref.py.

k_lsop8_reconstruct walks bands of 64 rows, a lane per row, and hands two seam rows to the next band through LDS: tiles of two and
three bands, last bands of one, two and exactly 64 rows, narrow tiles (lane 63 writes its seam after lane 0 has finished) and wide
ones (it writes while lane 0 reads), the widths around its 16-byte block accesses, the dynamic-LDS opt-in above 8,192 columns and
the column limit itself.  k_lsop8_predict strides over the interior with dr = STEP / wI, dc = STEP - dr * wI, STEP = 128 and 256:
interior widths of 128 and 256 (dc = 0) and beyond 256 (dr = 0).  Every shape runs a batch of kinds, one of them on the
scan-order-sum route, so that tiles also start at every alignment an odd cell count gives.  Then the switch between the exact and
the scan-order sums, one unit either side of max|v|^2 * interior cells = 2^53 (tests/lsop08_cases.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import lsop08_cases as K
import lsop08_ref as R
from tilegen import make_tile

pytestmark = pytest.mark.gpu

OK, DECLINED, ERR_UNSUPPORTED = 0, 1, -7
KINDS = ("terrain0", "noise16", "noise32", "sparse_big", "smooth")       # noise32: max|v|^2 * cells >= 2^53, the scan-order sums

ROW_SHAPES = [(67, 5), (68, 5), (130, 5), (131, 5), (195, 6), (67, 70), (131, 70), (194, 65)]
COL_SHAPES = [(4, 130), (5, 131), (4, 258), (5, 259), (6, 300), (4, 515), (5, 9), (5, 10), (5, 11)]
WIDE_SHAPES = {(4, 8193): "terrain0", (4, 16384): "sparse_big"}         # one kind each; the second one on the scan-order route


def _random_shape(seed):
    rng = np.random.default_rng(seed)
    return int(rng.integers(4, 141)), int(rng.integers(4, 301))


RANDOM_SEEDS = list(range(101, 113))
assert all(4 <= nr <= 140 and 4 <= nc <= 300 for nr, nc in map(_random_shape, RANDOM_SEEDS))
assert any(nr > 66 for nr, _ in map(_random_shape, RANDOM_SEEDS)) and any(nr * nc % 4 for nr, nc in map(_random_shape, RANDOM_SEEDS))
ids = lambda s: "%dx%d" % s


@pytest.fixture(scope="module")
def codec():
    import gridfour_amd
    return gridfour_amd.LsCodec08Hip()


def tile(kind, nr, nc):
    return R.terrain(nr, nc, int(kind[7:])) if kind.startswith("terrain") else make_tile(kind, nr, nc)


@functools.lru_cache(maxsize=None)
def ref(kind, nr, nc):
    """(tile, predict() or None, type-0 packing, type-1 packing) by the restatement, once per module"""
    v = tile(kind, nr, nc)
    pr = R.predict(nr, nc, v)
    if pr is None:
        return v, None, None, None
    return v, pr, R.container(6, *pr, ctype=0)[0], R.container(6, *pr, ctype=1)[0]


def _all_four(codec, nr, nc, kinds):
    """predict, reconstruct, the device encoder and the device decoder (both container types) on one batch of kinds"""
    refs = [ref(k, nr, nc) for k in kinds]
    tiles = np.stack([r[0] for r in refs])
    assert any(K.bound(nr, nc, r[0]) >= K.TWO53 for r in refs) or len(kinds) == 1
    seeds, coefs, res, status = codec.predict(nr, nc, tiles)
    packs, est = codec.encode_batch_dev(6, nr, nc, tiles)
    good = []
    for t, k in enumerate(kinds):
        v, pr, p0, p1 = refs[t]
        if pr is None:
            assert status[t] == DECLINED and est[t] == DECLINED and packs[t] is None, k
            continue
        seed, u, init, inter = pr
        assert status[t] == OK and seeds[t] == seed, (k, status[t])
        assert coefs[t].tobytes() == u.tobytes(), (k, coefs[t], u)
        got = res[t].tolist()
        assert got[:len(init)] == init, (k, "initialisers")
        bad = np.nonzero(np.array(got[len(init):]) != np.array(inter))[0]
        assert bad.size == 0, (k, "interior", bad[:8].tolist())
        assert est[t] == OK and packs[t] == p0, (k, est[t], len(packs[t] or b""), len(p0))
        good.append(t)
    assert len(good) >= min(3, len(kinds)), [kinds[t] for t in good]
    prs = [refs[t][1] for t in good]
    got, st = codec.reconstruct(nr, nc, [p[0] for p in prs], np.stack([p[1] for p in prs]), np.array([p[2] + p[3] for p in prs], np.int32))
    for i, t in enumerate(good):
        bad = np.nonzero(got[i] != tiles[t])[0]
        assert st[i] == OK and bad.size == 0, (kinds[t], "reconstruct", st[i], [(int(b) // nc, int(b) % nc) for b in bad[:8]])
    batch = [refs[t][2] for t in good] + [refs[t][3] for t in good]
    vals, st = codec.decode_batch_dev(nr, nc, batch)
    for i, t in enumerate(good + good):
        assert st[i] == OK and np.array_equal(vals[i], tiles[t]), (kinds[t], "decode type %d" % (i >= len(good)), st[i])


@pytest.mark.parametrize("shape", ROW_SHAPES, ids=ids)
def test_band_seams(codec, shape):
    """two and three bands; a last band of one row (67), two (68, 195: the third band's), exactly 64 after another (130) or two
    (194); 5 and 6 columns: lane 63 writes its seam after lane 0 has finished; 65 and 70: while lane 0 reads"""
    _all_four(codec, *shape, KINDS)


@pytest.mark.parametrize("shape", COL_SHAPES, ids=ids)
def test_column_strides(codec, shape):
    """interior widths 128 and 256 (dc = 0 in the 128- and the 256-strided walk), 129 and 257, 298 and 513 (dr = 0); 9, 10 and 11
    columns: a row is one block of eight steps and a partial one, so that a lane's 16-byte accesses (a whole block inside the row:
    c0 >= 2 and c0 + 8 <= nC for the residuals, c0 >= 0 for the values) and its single ones both occur, lane by lane differently"""
    _all_four(codec, *shape, KINDS)


@pytest.mark.parametrize("seed", RANDOM_SEEDS, ids=lambda s: "seed%d-%dx%d" % ((s,) + _random_shape(s)))
def test_random_shapes(codec, seed):
    _all_four(codec, *_random_shape(seed), KINDS)


@functools.lru_cache(maxsize=None)
def wide_ref(nr, nc):
    """the restatement on a tile at the width limit (its scalar reconstruct: about 33,000 interior cells, a second or two)"""
    v, pr, p0, p1 = ref(WIDE_SHAPES[(nr, nc)], nr, nc)
    seed, u, init, inter = pr
    back = R.reconstruct(nr, nc, seed, init, inter, u)
    assert np.array_equal(back, v)
    return back


@pytest.mark.parametrize("shape", list(WIDE_SHAPES), ids=ids)
def test_width_limit(codec, shape):
    """8,193 columns: the first width whose two seam rows need more than 64 KiB of LDS (the launcher's opt-in); 16,384: the limit"""
    nr, nc = shape
    kind = WIDE_SHAPES[shape]
    assert 2 * nc * 4 > 65536 and (K.bound(nr, nc, ref(kind, nr, nc)[0]) >= K.TWO53) == (kind == "sparse_big")
    want = wide_ref(nr, nc)
    _all_four(codec, nr, nc, (kind,))
    seed, u, init, inter = ref(kind, nr, nc)[1]
    got, st = codec.reconstruct(nr, nc, [seed], u[None, :], np.array([init + inter], np.int32))
    assert st[0] == OK and np.array_equal(got[0], want)


@pytest.mark.parametrize("shape", [(4, 16385), (8192, 8192)], ids=ids)
def test_shapes_beyond_the_limit_are_refused(codec, shape):
    """More than 16,384 columns, or 2^26 cells: GF_ERR_UNSUPPORTED from every entry point, and nothing written.

    EVERY device and host array below is token-sized -- 256 bytes where a real call needs up to a gigabyte (values, residuals, slots,
    the blob).  That is safe only because each entry point answers before it launches, copies or stages anything: in
    gvrs_api_lsop.hip the shape test follows the argument checks directly in gf_lsop08_predict_dev (which the device encoder calls
    before its packer), gf_lsop08_reconstruct_dev and lsop08DecodeDev (before its two memsets), and lsopEncodeBatchHost /
    lsopDecodeBatchHost test hostFormsCheckShape before they size their staging.  The sentinel in every array shows it."""
    from gridfour_amd import DeviceBuffer, lib
    L = lib()
    nr, nc = shape
    assert nc > 16384 or nr * nc >= 2 ** 26
    n = int(L.gf_lsop08_residual_count(nr, nc))
    assert n == R.n_init(nr, nc) + R.n_interior(nr, nc)
    stride = (n + 3) // 4 * 4
    ctx = codec.ctx
    dev = DeviceBuffer(ctx, 4 * 256).fill(0x5A)
    a, b, c, d = (C.c_void_p(dev.ptr.value + 256 * i) for i in range(4))
    h = ctx.handle
    rcs = {"predict_dev": L.gf_lsop08_predict_dev(h, nr, nc, 1, a, b, stride, c, d),
           "reconstruct_dev": L.gf_lsop08_reconstruct_dev(h, nr, nc, 1, b, stride, c, None, a, d),
           "encode_batch_i32_dev": L.gf_lsop08_encode_batch_i32_dev(h, 0, nr, nc, 1, a, b, 64, c, d, b, stride, c, d),
           "decode_batch_i32_dev": L.gf_lsop08_decode_batch_i32_dev(h, nr, nc, 1, a, 64, None, 64, c, b, d, b, stride, c, d)}
    ctx.synchronize()
    assert (dev.download(np.uint8, 4 * 256) == 0x5A).all(), "a refused call wrote to device memory"
    host = np.full(256, 0x5A, np.uint8)
    vals, blob, types, status = (host[64 * i:64 * (i + 1)] for i in range(4))
    ptr = lambda x: C.c_void_p(x.ctypes.data)
    off = np.array([0, 64], np.uint64)
    out_len = C.c_size_t(0)
    rcs["encode_batch_i32"] = L.gf_lsop08_encode_batch_i32(h, 0, nr, nc, 1, ptr(vals), ptr(blob), 64, ptr(off), ptr(types), ptr(status))
    rcs["decode_batch_i32"] = L.gf_lsop08_decode_batch_i32(h, nr, nc, 1, ptr(blob), ptr(off), ptr(vals), ptr(status))
    rcs["encode_i32"] = L.gf_lsop08_encode_i32(h, 0, nr, nc, ptr(vals), ptr(blob), 64, C.byref(out_len))
    rcs["decode_i32"] = L.gf_lsop08_decode_i32(h, nr, nc, ptr(blob), 64, ptr(vals))
    assert all(rc == ERR_UNSUPPORTED for rc in rcs.values()), rcs
    assert (host == 0x5A).all() and off.tolist() == [0, 64] and out_len.value == 0
    dev.free()


# ---- the exact / scan-order switch
@pytest.mark.parametrize("shape", [(4, 4), (66, 66)], ids=ids)
def test_sum_route_threshold(codec, shape):
    """max|v|^2 * interior cells one unit under 2^53 (27 FMA accumulators a thread, any order) and one unit over (54 threads, the
    reference's scan order), the magnitude that decides in the interior, in row 0 and in the last cell; a tile holding INT32_MIN
    (its magnitude, 2^31, does not fit an int32)"""
    nr, nc = shape
    tiles = K.threshold_tiles(nr, nc)
    names = sorted(tiles)
    for name in names:                                                     # from Python integers, before any GPU call
        m = max(abs(int(x)) for x in tiles[name])
        assert (m * m * R.n_interior(nr, nc) < 2 ** 53) == name.startswith("at-"), name
    seeds, coefs, res, status = codec.predict(nr, nc, np.stack([tiles[k] for k in names]))
    for t, name in enumerate(names):
        seed, u, init, inter = R.predict(nr, nc, tiles[name])
        assert status[t] == OK and seeds[t] == seed, (name, status[t])
        assert coefs[t].tobytes() == u.tobytes(), (name, coefs[t], u)
        assert res[t].tolist() == init + inter, name


def test_scan_order_sums_on_a_wide_tile(codec):
    """the scan-order route where a row of the interior is wider than the exact route's stride: 6 x 300, values over the int32 range"""
    nr, nc = 6, 300
    v = np.random.default_rng(300).integers(-2 ** 31, 2 ** 31, nr * nc).astype(np.int32)
    assert K.bound(nr, nc, v) >= 2 ** 53
    seed, u, init, inter = R.predict(nr, nc, v)
    seeds, coefs, res, status = codec.predict(nr, nc, v[None, :])
    assert status[0] == OK and seeds[0] == seed and coefs[0].tobytes() == u.tobytes() and res[0].tolist() == init + inter
