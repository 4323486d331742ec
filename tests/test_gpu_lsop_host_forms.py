"""The host-memory entry points of LSOP12 and LSOP08 (gf_lsop12_* / gf_lsop08_*_batch_i32 of the C ABI) where no other test pins
them: tiles below the family's smallest side, a blob one byte too small, a decreasing offsets array, an unknown flag bit and
LSOP08's shape limit.  The batches are those of test_lsop_container_header.py (lsop_container_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import lsop_container_cases as K

pytestmark = pytest.mark.gpu

OK, DECLINED, ERR_BOUNDS, ERR_CAPACITY, ERR_ARG, ERR_UNSUPPORTED = 0, 1, -2, -3, -4, -7
FAMILIES = [12, 8]
SMALL = {12: [(5, 6), (6, 5)], 8: [(3, 4), (4, 3)]}
CAPACITY_BATCH = {12: "lsop12_48", 8: "lsop08_7x9"}


@pytest.fixture(scope="module")
def ctx():
    import gridfour_amd
    return gridfour_amd.GvrsHipContext()


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _fn(family, name):
    from gridfour_amd import lib
    return getattr(lib(), "gf_lsop%02d_%s" % (family, name))


def encode(ctx, family, nr, nc, values, flags, cap):
    """the host encoder on outputs filled with other values: (return value, blob, offsets, types, statuses)"""
    nt = values.shape[0]
    blob, offsets = np.full(max(cap, 1), 0xEE, np.uint8), np.full(nt + 1, 0xFFFFFFFFFFFFFFFF, np.uint64)
    types, status = np.full(nt, 9, np.uint8), np.full(nt, 99, np.int32)
    v = np.ascontiguousarray(values, np.int32)
    head = (ctx.handle, K.CODEC_INDEX, nr, nc, nt, _ptr(v)) + ((flags,) if family == 12 else ())
    rc = _fn(family, "encode_batch_i32")(*head, _ptr(blob), cap, _ptr(offsets), _ptr(types), _ptr(status))
    return rc, blob, offsets.tolist(), types.tolist(), status.tolist()


def decode(ctx, family, nr, nc, blob, offsets):
    nt = len(offsets) - 1
    values, status = np.zeros((nt, nr * nc), np.int32), np.full(nt, 99, np.int32)
    blob = np.frombuffer(bytes(blob) + b"\0" * 16, np.uint8)
    rc = _fn(family, "decode_batch_i32")(ctx.handle, nr, nc, nt, _ptr(blob), _ptr(np.array(offsets, np.uint64)), _ptr(values), _ptr(status))
    return rc, values, status.tolist()


@pytest.mark.parametrize("family,shape", [(f, s) for f in FAMILIES for s in SMALL[f]], ids=lambda x: str(x).replace(" ", ""))
def test_tile_below_the_smallest_side(ctx, family, shape):
    nr, nc = shape
    values = np.arange(3 * nr * nc, dtype=np.int32).reshape(3, -1) * 7
    rc, blob, offsets, types, status = encode(ctx, family, nr, nc, values, 1, 4096)
    assert rc == OK and offsets == [0, 0, 0, 0] and status == [DECLINED] * 3 and types == [0] * 3
    assert (blob == 0xEE).all()
    rc, _, status = decode(ctx, family, nr, nc, bytes(96), [0, 32, 64, 96])
    assert rc == OK and status == [ERR_BOUNDS] * 3


@pytest.mark.parametrize("family", FAMILIES)
def test_blob_one_byte_short(ctx, family):
    b = K.batch(CAPACITY_BATCH[family])
    want_blob, want_offsets, want_types, want_status = b.want_blob()
    total = len(want_blob)
    rc, blob, offsets, types, status = encode(ctx, family, b.nr, b.nc, b.values, b.flags, total)
    assert rc == OK and bytes(blob[:total]) == want_blob
    assert (offsets, types, status) == (want_offsets, want_types, want_status)
    rc, blob, offsets, types, status = encode(ctx, family, b.nr, b.nc, b.values, b.flags, total - 1)
    assert rc == ERR_CAPACITY and (blob == 0xEE).all()
    assert (offsets, types, status) == (want_offsets, want_types, want_status)


@pytest.mark.parametrize("family", FAMILIES)
def test_decode_refuses_decreasing_offsets(ctx, family):
    b = K.batch(CAPACITY_BATCH[family])
    first, last = b.tiles[0].want, b.tiles[2].want                    # the two good tiles
    rc, values, status = decode(ctx, family, b.nr, b.nc, first + last, [0, len(first), len(first) + len(last)])
    assert rc == OK and status == [OK, OK] and np.array_equal(values, b.values[[0, 2]])
    rc, _, status = decode(ctx, family, b.nr, b.nc, first + last, [0, len(first) + len(last), len(first)])
    assert rc == ERR_ARG and status == [99, 99]


def test_lsop12_refuses_an_unknown_flag_bit(ctx):
    b = K.batch("lsop12_6")
    for flags in (4, 5, 7):
        rc, _, _, _, _ = encode(ctx, 12, b.nr, b.nc, b.values, flags, 4096)
        assert rc == ERR_ARG, flags


def test_lsop08_refuses_more_than_16384_columns(ctx):
    import gridfour_amd
    from gridfour_amd import lib
    nr, nc = 4, 16385
    values = np.zeros((1, nr * nc), np.int32)
    rc, _, _, _, _ = encode(ctx, 8, nr, nc, values, 0, 1 << 20)
    assert rc == ERR_UNSUPPORTED
    rc, _, _ = decode(ctx, 8, nr, nc, bytes(64), [0, 64])
    assert rc == ERR_UNSUPPORTED
    n = int(lib().gf_lsop08_residual_count(nr, nc))
    stride = (n + 3) // 4 * 4
    dv, dr = gridfour_amd.DeviceBuffer(ctx, values.nbytes).fill(0), gridfour_amd.DeviceBuffer(ctx, stride * 4 + 16).fill(0)
    dc, ds = gridfour_amd.DeviceBuffer(ctx, 64).fill(0), gridfour_amd.DeviceBuffer(ctx, 16).fill(0)
    try:
        assert lib().gf_lsop08_predict_dev(ctx.handle, nr, nc, 1, dv.ptr, dr.ptr, stride, dc.ptr, ds.ptr) == ERR_UNSUPPORTED
        assert lib().gf_lsop08_reconstruct_dev(ctx.handle, nr, nc, 1, dr.ptr, stride, dc.ptr, None, dv.ptr, ds.ptr) == ERR_UNSUPPORTED
    finally:
        for d in (dv, dr, dc, ds):
            d.free()
