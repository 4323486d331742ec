"""The byte path's rows and pool move (gvrs_decode.hip: m32_bytes_rows, pool_to_m32) at the shapes and values that decide them.

The rows sum a lane's four residual bytes with dot products (v_dot4_i32_i8), Triangle down the rows first and over the lanes
second, a block of up to 16 rows kept in registers between the pre-pass and the rows; the pool move goes in trips of four
words.  Every case is built FROM its residual stream -- one byte per residual, -126 ... 126, so that the tree holds no
introducer (0x7f / 0x81) and no null code (0x80) --, turned into cells by the oracle's inverse predictor, encoded by the
oracle with that predictor forced, decoded on the GPU through gf_huffman_decode_batch_i32_dev in batches of 3 - 8 tiles and
compared cell by cell.  That the byte path is what runs is checked on the CPU before the GPU call (byte_path_stream)."""
import ctypes as C

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -(2 ** 31)
COLS = [4, 5, 6, 7, 8, 149, 150, 151, 253, 254, 255, 256]       # the partial last lane (rem 1 - 3), the headline's, the last eligible
ROWS = [2, 3, 7, 8, 9, 64, 65, 68, 129]                         # fewer rows than waves; 15 / 16 / 17 rows a block (256 threads); the third
#                                                                 trip of the column-0 scan
SHAPES = [(9, c) for c in COLS] + [(r, 8) for r in ROWS] + [
    (120, 150),                                                 # 512 threads, 15 rows a block
    (160, 160),                                                 # 1,024 threads, 10 rows a block
    (256, 16), (272, 16),                                       # 1,024 threads, 16 and 17 rows a block
    (256, 256)]                                                 # 255 rows of 256 columns: Triangle's accumulators pass 2^23


@pytest.fixture(scope="module")
def ctx():
    import gridfour_amd
    return gridfour_amd.GvrsHipContext(0)


def byte_path_stream(model, n_rows, n_cols, cells):
    """The M32 stream of `cells` under `model`, after asserting what sends a tile down the byte path: one byte per residual and
    none of them 0x7f, 0x80 or 0x81 (the Huffman tree's leaves are the bytes that occur)."""
    m32, _ = oracle.predictor_encode(model, n_rows, n_cols, cells)
    assert m32 is not None and len(m32) == n_rows * n_cols - 1, (model, n_rows, n_cols, m32 and len(m32))
    assert not set(m32) & {0x7f, 0x80, 0x81}
    return m32


def tile_from_residuals(model, seed, n_rows, n_cols, res):
    """Cells whose residual stream under `model` is `res` (int8 values, stream order), all of them valid int32 that no sum wrapped to."""
    res = np.asarray(res, np.int8)
    assert res.size == n_rows * n_cols - 1 and np.abs(res.astype(np.int32)).max() <= 126
    cells = oracle.predictor_decode(model, seed, n_rows, n_cols, res.tobytes())
    grid = cells.astype(np.int64).reshape(n_rows, n_cols)
    assert (cells != INT32_MIN).all()
    for axis in (0, 1):                                        # a wrapped sum shows as a step of 2^32 between neighbours
        assert np.abs(np.diff(grid, axis=axis)).max() < 2 ** 24
    assert byte_path_stream(model, n_rows, n_cols, cells) == res.tobytes()
    return cells


def value_tiles(model, n_rows, n_cols):
    n = n_rows * n_cols - 1
    rng = np.random.default_rng(1000 * n_rows + n_cols + model)
    alt = np.where(np.arange(n) & 1, -126, 126)
    return np.stack([
        tile_from_residuals(model, 5, n_rows, n_cols, np.full(n, 126)),           # the largest in-lane and cross-lane sums
        tile_from_residuals(model, -5, n_rows, n_cols, np.full(n, -126)),
        tile_from_residuals(model, 77, n_rows, n_cols, alt),
        tile_from_residuals(model, -77, n_rows, n_cols, -alt),
        # sums that wrap through 2^31 inside the accumulators while the cells themselves stay in range: falling from INT32_MAX, rising
        # from INT32_MIN + 1
        tile_from_residuals(model, INT32_MAX - 3, n_rows, n_cols, rng.integers(-126, 1, n)),
        tile_from_residuals(model, INT32_MIN + 1 + 3, n_rows, n_cols, rng.integers(0, 127, n)),
        tile_from_residuals(model, 123456, n_rows, n_cols, rng.integers(-126, 127, n))])


def decode_dev(ctx, n_rows, n_cols, packs):
    """The packings through gf_huffman_decode_batch_i32_dev, as one blob with offsets."""
    from gridfour_amd import DeviceBuffer, lib
    from gridfour_amd._lib import check
    nt, cells = len(packs), n_rows * n_cols
    lengths = np.array([len(p) for p in packs], np.uint32)
    starts = np.concatenate([[0], np.cumsum((lengths.astype(np.int64) + 3) // 4 * 4)]).astype(np.uint64)
    blob = np.zeros(int(starts[-1]) + 64, np.uint8)
    for t, p in enumerate(packs):
        blob[int(starts[t]):int(starts[t]) + len(p)] = np.frombuffer(p, np.uint8)
    ctx.reserve(n_rows, n_cols, nt)
    d_blob, d_off, d_len = DeviceBuffer(ctx, blob.size), DeviceBuffer(ctx, (nt + 1) * 8), DeviceBuffer(ctx, nt * 4)
    d_val, d_st = DeviceBuffer(ctx, nt * cells * 4), DeviceBuffer(ctx, nt * 4)
    try:
        d_blob.upload(blob)
        d_off.upload(starts)
        d_len.upload(lengths)
        d_val.fill(0x5a)
        d_st.fill(0x5a)
        check(lib().gf_huffman_decode_batch_i32_dev(ctx.handle, None, n_rows, n_cols, nt, d_blob.ptr, blob.size, d_off.ptr, 0, d_len.ptr,
                                                    d_val.ptr, d_st.ptr), "gf_huffman_decode_batch_i32_dev")
        ctx.synchronize()
        return d_val.download(np.int32, nt * cells).reshape(nt, cells), d_st.download(np.int32, nt)
    finally:
        for b in (d_blob, d_off, d_len, d_val, d_st):
            b.free()


def check_batch(ctx, model, n_rows, n_cols, tiles):
    packs = []
    for v in tiles:
        ref, used = oracle.codec_huffman_encode(0, n_rows, n_cols, v, predictor_mask=1 << (model - 1))
        assert ref is not None and used == model
        packs.append(ref)
    vals, st = decode_dev(ctx, n_rows, n_cols, packs)
    assert (st == 0).all(), (model, st)
    for t, v in enumerate(tiles):
        if not np.array_equal(vals[t], v):
            bad = np.nonzero(vals[t] != v)[0]
            raise AssertionError("model %d tile %d: %d cells differ, first at %d (row %d col %d): got %d want %d" % (
                model, t, bad.size, bad[0], bad[0] // n_cols, bad[0] % n_cols, vals[t][bad[0]], v[bad[0]]))


@pytest.mark.parametrize("model", [1, 2, 3], ids=["differencing", "linear", "triangle"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_rows_at_their_shapes_and_extreme_sums(ctx, shape, model):
    n_rows, n_cols = shape
    check_batch(ctx, model, n_rows, n_cols, value_tiles(model, n_rows, n_cols))


# ---- the pool move: symbols per subsequence of the fast pass, known on the CPU -------------------------------------------------
POOL_SHAPE = (120, 150)
MIN_UNIT, MAXQ_512 = 128, 512                                   # gvrs_decode.hip: GF_DEC_MIN_UNIT; subsequences of the 512-thread build


def symbols_per_subsequence(packing, m32):
    """How many symbols START in each subsequence of the text, the way huffman_to_m32_fast cuts it (unit: the text's bits over
    MAXQ, rounded up to 32, at least GF_DEC_MIN_UNIT).  The code lengths come from the oracle's encoder, whose output must be
    the packing's own bits."""
    data, end, cl, tree_bits = oracle.huffman_encode(m32, bit_pos=80, prefix=packing[:10])
    assert data == packing
    text_bits = end - 80 - tree_bits
    unit = max(MIN_UNIT, ((text_bits + MAXQ_512 - 1) // MAXQ_512 + 31) // 32 * 32)
    q = max(1, (text_bits + unit - 1) // unit)
    lens = cl[np.frombuffer(m32, np.uint8)].astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return np.bincount(starts // unit, minlength=q)


def pool_tiles():
    """Three Differencing tiles of 120 x 150 and the symbol counts of their subsequences."""
    n_rows, n_cols = POOL_SHAPE
    n = n_rows * n_cols - 1
    rng = np.random.default_rng(42)
    # 1: a residual of one bit and 51 of two others (two bits each): 17,999 + 51 = 141 x 128 + 2 bits of text, so the LAST subsequence
    # holds two symbols
    a = np.zeros(n, np.int64)
    a[100:126] = 1
    a[300:325] = 2
    # 2: two residuals, one bit each: every subsequence holds 128 symbols, 32 words, its whole share of the pool
    b = rng.integers(0, 2, n)
    # 3: frequencies cut for code lengths of 1 bit (0), 3 bits (1), 4 bits (10 .. 13) and 7 bits (-60 .. -45), 48 K bits in all (a
    # unit of 128 bits): a run of seven-bit codes (18 - 19 symbols a subsequence: 5 words), a run of four-bit codes (32: 8 words),
    # a run of 3 + 4 + 4 bits (34 - 35: 9 words), the rest one-bit codes
    n1, n2, n3 = 1850, 400, 6750
    k = np.arange(n3)
    c = np.concatenate([np.arange(-60, -44)[np.arange(n1) % 16], np.arange(10, 14)[np.arange(n2) % 4],
                        np.where(k % 3 == 0, 1, np.arange(10, 14)[(k - k // 3 - 1) % 4]), np.zeros(n - n1 - n2 - n3, np.int64)])
    tiles, counts = [], []
    for res in (a, b, c):
        v = tile_from_residuals(1, 1000, n_rows, n_cols, res)
        pack, used = oracle.codec_huffman_encode(0, n_rows, n_cols, v, predictor_mask=1)
        assert used == 1
        tiles.append(v)
        counts.append(symbols_per_subsequence(pack, res.astype(np.int8).tobytes()))
    return np.stack(tiles), counts


def test_pool_move_at_the_trip_size(ctx):
    """The symbols of a subsequence leave the pool in trips of four words.  A subsequence of 128 bits and more cannot hold fewer
    than four symbols unless it is the text's last, so the "no whole word" case (0 - 3 symbols: head and tail bytes only) is the
    first tile's last subsequence; the second tile fills every share to its last slot (128 symbols, 32 words, a multiple of four);
    the third has subsequences of 5, 8 and 9 words, on either side of the trip size."""
    tiles, counts = pool_tiles()
    assert 1 <= counts[0][-1] <= 3, counts[0][-4:]
    assert (counts[1][:-1] == 128).all() and counts[1].size > 100
    words = set((counts[2] + 3) // 4)
    assert {5, 8, 9} <= words, sorted(words)
    assert max(c.max() for c in counts) <= 128                  # no share of the pool overflows: the pool move is what runs
    check_batch(ctx, 1, POOL_SHAPE[0], POOL_SHAPE[1], tiles)
