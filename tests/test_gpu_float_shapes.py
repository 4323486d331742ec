"""k_float_planes_encode / k_float_planes_decode / k_float_short_planes away from their usual shapes, bit for bit against the
oracle (whose agreement with an independent numpy restatement at these very shapes is pinned by tests/test_float_ref.py).

What the shapes are for:
  * The decode kernel walks the rows in chunks of 1,024; wave 0 decodes the column-0 chain of a chunk into LDS and three carries
    cross into the next chunk.  (1023,5) (1024,8) (1025,1) (1025,4) (2049,3) (2050,4) lie on both sides of the first and the
    second seam, on either kernel path; (3,131) and (2,1028) take several column trips per row on either path.
  * Both kernels take four cells per lane when nCols % 4 == 0 AND the value pointer is 16-byte aligned; the ABI asks only for
    float alignment, so a multiple-of-four column count must also go through the one-cell path: value pointers at +4, +8, +12.
  * The planes of a tile follow one another without padding: plane strides of exactly gf_float_planes_bytes (odd at (3,7),
    (5,4) and (1025,1)), and that + 1 and + 3; whatever lies between two tiles' planes and behind the last tile keeps its fill byte.
  * k_float_short_planes restates Java's single scratch array for planes that inflate short: one thread per tile walks the
    tile, at the one-cell path (7,9), the tall one-cell path (1025,3) and the tall four-cell path (1030,4).
"""
import numpy as np
import pytest

import float_ref
import oracle
from test_gpu_float import _float_tiles

pytestmark = pytest.mark.gpu

FILL = 0xAB                                      # plane buffers before the encode
GUARD_BYTE = 0x5C                                # value and status buffers before a decode
BAND = 256                                       # bytes of guard on either side


@pytest.fixture(scope="module")
def fcodec():
    import gridfour_amd
    return gridfour_amd.CodecFloatHip(level=6)


def _tiles(n_rows, n_cols):
    """The five kinds of test_gpu_float.py, random 32-bit patterns (every byte sum wraps) and the column-0 chain tile; uint32"""
    rng = np.random.default_rng(n_rows * 1000 + n_cols)
    kinds = [t.view(np.uint32) for t in _float_tiles(rng, n_rows, n_cols)]
    return np.stack(kinds + [float_ref.random_bits(rng, n_rows, n_cols), float_ref.chain_bits(n_rows, n_cols)])


def _planes_encode(ctx, n_rows, n_cols, tiles, stride, value_offset=0):
    """gf_float_planes_encode_dev reading the cells at `value_offset` bytes behind a 16-byte aligned base: the planes [nt, stride].
    The plane buffer is FILL before the call; what is not plane must still be FILL afterwards, a band behind the last tile too."""
    from gridfour_amd import DeviceBuffer, lib
    from gridfour_amd._lib import check
    L = lib()
    nt = tiles.shape[0]
    pb = int(L.gf_float_planes_bytes(n_rows, n_cols))
    d_vals = DeviceBuffer(ctx, tiles.nbytes + 16).upload(tiles, value_offset)
    d_planes = DeviceBuffer(ctx, nt * stride + BAND).fill(FILL)
    check(L.gf_float_planes_encode_dev(ctx.handle, None, n_rows, n_cols, nt, d_vals.ptr.value + value_offset, d_planes.ptr, stride),
          "gf_float_planes_encode_dev")
    ctx.synchronize()
    raw = d_planes.download(np.uint8, nt * stride + BAND)
    planes = raw[:nt * stride].reshape(nt, stride)
    assert (planes[:, pb:] == FILL).all(), "bytes between two tiles' planes were written"
    assert (raw[nt * stride:] == FILL).all(), "bytes behind the last tile's planes were written"
    d_vals.free()
    return planes, d_planes


def _planes_decode(ctx, n_rows, n_cols, nt, d_planes, stride, value_offset=0):
    """gf_float_planes_decode_dev writing the cells at `value_offset` bytes behind a 16-byte aligned base, guard bands on both
    sides of them: the raw bits [nt, n]."""
    from gridfour_amd import DeviceBuffer, lib
    from gridfour_amd._lib import check
    nbytes = nt * n_rows * n_cols * 4
    d_back = DeviceBuffer(ctx, BAND + nbytes + 16 + BAND).fill(GUARD_BYTE)
    check(lib().gf_float_planes_decode_dev(ctx.handle, None, n_rows, n_cols, nt, d_planes.ptr, stride,
                                           d_back.ptr.value + BAND + value_offset), "gf_float_planes_decode_dev")
    ctx.synchronize()
    raw = d_back.download(np.uint8, d_back.nbytes)
    lo, hi = BAND + value_offset, BAND + value_offset + nbytes
    assert (raw[:lo] == GUARD_BYTE).all() and (raw[hi:] == GUARD_BYTE).all(), "cells written outside the tiles"
    d_back.free()
    return raw[lo:hi].copy().view(np.uint32).reshape(nt, -1)


def _dev_decode(ctx, n_rows, n_cols, packs, value_offset=0):
    """gf_float_decode_batch_f32_dev on packings in device memory, guard bands around the cells and behind the statuses:
    (raw bits [nt, n], status)."""
    from gridfour_amd import DeviceBuffer, lib
    from gridfour_amd._lib import check
    nt, n = len(packs), n_rows * n_cols
    lens = np.array([len(p) for p in packs], np.uint32)
    offs = np.zeros(nt + 1, np.uint64)
    offs[1:] = np.cumsum(lens, dtype=np.uint64)
    blob = np.frombuffer(b"".join(packs) + bytes(32), np.uint8)
    d_blob = DeviceBuffer(ctx, blob.nbytes).upload(blob)
    d_off = DeviceBuffer(ctx, offs.nbytes).upload(offs)
    d_len = DeviceBuffer(ctx, lens.nbytes + 16).upload(lens)
    d_vals = DeviceBuffer(ctx, BAND + nt * n * 4 + 16 + BAND).fill(GUARD_BYTE)
    d_st = DeviceBuffer(ctx, nt * 4 + BAND).fill(GUARD_BYTE)
    check(lib().gf_float_decode_batch_f32_dev(ctx.handle, None, n_rows, n_cols, nt, d_blob.ptr, blob.nbytes, d_off.ptr, d_len.ptr,
                                              d_vals.ptr.value + BAND + value_offset, d_st.ptr), "gf_float_decode_batch_f32_dev")
    ctx.synchronize()
    raw = d_vals.download(np.uint8, d_vals.nbytes)
    st_raw = d_st.download(np.uint8, d_st.nbytes)
    lo, hi = BAND + value_offset, BAND + value_offset + nt * n * 4
    st = st_raw[:nt * 4].copy().view(np.int32)
    assert (st_raw[nt * 4:] == GUARD_BYTE).all(), "status written past the last tile"
    # (a tile that fails may leave its cells as they were; nothing outside the tiles may change)
    assert (raw[:lo] == GUARD_BYTE).all() and (raw[hi:] == GUARD_BYTE).all(), "cells written outside the tiles"
    for b in (d_blob, d_off, d_len, d_vals, d_st):
        b.free()
    return raw[lo:hi].copy().view(np.uint32).reshape(nt, n), st


def _stride16(n_rows, n_cols):
    from gridfour_amd import lib
    return (int(lib().gf_float_planes_bytes(n_rows, n_cols)) + 15) // 16 * 16


TALL = [(1023, 5), (1024, 8), (1025, 1), (1025, 4), (2049, 3), (2050, 4), (3, 131), (2, 1028)]


@pytest.mark.parametrize("shape", TALL, ids=lambda s: "%dx%d" % s)
def test_tall_and_wide_tiles_match_oracle(fcodec, shape):
    """As test_planes_and_packings_match_oracle, across the 1,024-row seams and over several column trips: planes = oracle,
    planes -> bits, whole packings = oracle, decode = oracle through the host-memory batch and the device-resident one."""
    n_rows, n_cols = shape
    ctx = fcodec.ctx
    tiles = _tiles(n_rows, n_cols)
    nt = tiles.shape[0]
    stride = _stride16(n_rows, n_cols)
    planes, d_planes = _planes_encode(ctx, n_rows, n_cols, tiles, stride)
    for t in range(nt):
        ref = oracle.float_planes_encode(n_rows, n_cols, tiles[t])
        assert np.array_equal(planes[t, :ref.size], ref), (shape, t)
    back = _planes_decode(ctx, n_rows, n_cols, nt, d_planes, stride)
    bad = np.nonzero((back != tiles).any(axis=1))[0]
    assert bad.size == 0, (shape, bad, [int(np.nonzero(back[t] != tiles[t])[0][0]) // n_cols for t in bad])   # tile, first bad row
    d_planes.free()
    packs = fcodec.encode_floats_batch(2, n_rows, n_cols, tiles.view(np.float32))
    for t in range(nt):
        assert packs[t] == oracle.codec_float_encode(2, n_rows, n_cols, tiles[t], level=6), (shape, t)
        assert np.array_equal(oracle.codec_float_decode(n_rows, n_cols, packs[t]), tiles[t]), (shape, t)
    vals, st = fcodec.decode_floats_batch(n_rows, n_cols, packs)
    assert (st == 0).all() and np.array_equal(vals.view(np.uint32), tiles)
    dvals, dst = _dev_decode(ctx, n_rows, n_cols, packs)
    assert (dst == 0).all() and np.array_equal(dvals, tiles)


@pytest.mark.parametrize("offset", [4, 8, 12])
@pytest.mark.parametrize("shape", [(5, 12), (1030, 4)], ids=lambda s: "%dx%d" % s)
def test_value_pointer_aligned_for_float_only(fcodec, shape, offset):
    """nCols % 4 == 0 with a value pointer that is float-aligned but not 16-byte aligned: both kernels must take the one-cell
    path and give what the aligned run and the oracle give.  Encode reads from the offset pointer, decode writes to it, between
    guard bands."""
    n_rows, n_cols = shape
    ctx = fcodec.ctx
    tiles = _tiles(n_rows, n_cols)
    nt = tiles.shape[0]
    stride = _stride16(n_rows, n_cols)
    aligned, d_al = _planes_encode(ctx, n_rows, n_cols, tiles, stride)
    shifted, d_sh = _planes_encode(ctx, n_rows, n_cols, tiles, stride, offset)
    assert np.array_equal(shifted, aligned)
    for t in range(nt):
        ref = oracle.float_planes_encode(n_rows, n_cols, tiles[t])
        assert np.array_equal(shifted[t, :ref.size], ref), (shape, offset, t)
    assert np.array_equal(_planes_decode(ctx, n_rows, n_cols, nt, d_sh, stride), tiles)
    assert np.array_equal(_planes_decode(ctx, n_rows, n_cols, nt, d_sh, stride, offset), tiles)
    d_al.free()
    d_sh.free()
    packs = [oracle.codec_float_encode(2, n_rows, n_cols, tiles[t], level=6) for t in range(nt)]
    dvals, dst = _dev_decode(ctx, n_rows, n_cols, packs, offset)
    assert (dst == 0).all() and np.array_equal(dvals, tiles)


@pytest.mark.parametrize("extra", [0, 1, 3])
@pytest.mark.parametrize("shape", [(3, 3), (7, 9), (3, 7), (5, 4), (1025, 1)], ids=lambda s: "%dx%d" % s)
def test_plane_strides_that_are_no_multiple_of_16(fcodec, shape, extra):
    """Exactly gf_float_planes_bytes, and one and three bytes more.  The byte count is odd where the sign plane has an odd number
    of bytes -- (3,7) on the one-cell path, (5,4) on the four-cell path, (1025,1) across the row seam -- and even at (3,3) and
    (7,9), where + 1 and + 3 give the odd strides: the planes of every second tile begin at an odd address, on either path."""
    from gridfour_amd import lib
    n_rows, n_cols = shape
    ctx = fcodec.ctx
    tiles = _tiles(n_rows, n_cols)
    nt = tiles.shape[0]
    pb = int(lib().gf_float_planes_bytes(n_rows, n_cols))
    assert (pb % 2 == 1) == (shape in ((3, 7), (5, 4), (1025, 1)))
    stride = pb + extra
    planes, d_planes = _planes_encode(ctx, n_rows, n_cols, tiles, stride)
    for t in range(nt):
        assert np.array_equal(planes[t, :pb], oracle.float_planes_encode(n_rows, n_cols, tiles[t])), (shape, extra, t)
    assert np.array_equal(_planes_decode(ctx, n_rows, n_cols, nt, d_planes, stride), tiles)
    d_planes.free()


@pytest.mark.parametrize("shape", [(7, 9), (1025, 3), (1030, 4)], ids=lambda s: "%dx%d" % s)
def test_short_and_long_planes_match_oracle(fcodec, shape):
    """CodecFloat.decodeFloats inflates its five planes into ONE scratch array and decodes the mantissa deltas in place
    (CodecFloat.java:397-446): behind a plane that inflates short lies what the plane before left; a stream that holds more than
    the plane is cut at the room (Inflater.inflate(buf, 0, room)), no exception either way.  One plane short by
    keep in {0, 1, len // 3, len - 1} for each of the five planes, two planes short at once, and one plane 100 bytes long for
    each of the five; random 32-bit cells.  Device = oracle through both decode entry points."""
    n_rows, n_cols = shape
    bits = float_ref.random_bits(np.random.default_rng(n_rows * 31 + n_cols), n_rows, n_cols)
    good = fcodec.encodeFloats(3, n_rows, n_cols, bits.view(np.float32))
    assert good == oracle.codec_float_encode(3, n_rows, n_cols, bits, level=6)
    short, long = float_ref.damaged_plane_packings(good)
    packs = short + long + [good]
    want = [oracle.codec_float_decode(n_rows, n_cols, pk) for pk in packs]
    differs = sum(int(not np.array_equal(w, bits)) for w in want[:len(short)])
    assert differs >= len(short) - 2, differs                      # the short planes do change the tile: nothing passes vacuously
    for w in want[len(short):]:
        assert np.array_equal(w, bits)                             # the over-long ones decode to the intact tile
    vals, st = fcodec.decode_floats_batch(n_rows, n_cols, packs)
    dvals, dst = _dev_decode(fcodec.ctx, n_rows, n_cols, packs)
    for k in range(len(packs)):
        assert st[k] == 0 and np.array_equal(vals[k].view(np.uint32), want[k]), ("host batch", shape, k, int(st[k]))
        assert dst[k] == 0 and np.array_equal(dvals[k], want[k]), ("device batch", shape, k, int(dst[k]))
