"""GVRS file images updated in place on the GPU.  gf_file_update_block_elems_dev is held to the host-memory block form byte for byte,
on tile-aligned rectangles (nothing decoded, only enqueued) and on rectangles with partly covered tiles (the old records found by
k_file_locate and merged), with damaged old records, and both device forms are shown to return while a backlog still runs.  gf_file_update_records_dev is held to gf_file_update_assemble byte for byte (which
tests/test_file_update_assemble.py holds to the model) on every scenario of tests/file_update_cases.py, at the seams of the
allocator's 64-node turns in both of its routes (the list in LDS and in scratch, chosen by the capacity argument), at the seams of
the directory checksum's chunks (the table of tests/dir_seams.py, up to more than 64 chunks), and at one byte
too little room, where the image must stay as it was.  gf_file_update_block_elems, the host-memory block form, is held to the
model fed with its own records, and its images read back as the old raster with the rectangle replaced."""
import functools
import struct

import numpy as np
import pytest

import gridfour_amd
from gridfour_amd import GvrsFileHip, _lib

import file_update_cases as U
import gvrs_file_build as B
import gvrs_file_update_ref as R
import gvrs_file_write_ref as W
from dir_seams import SEAMS, read_chunk

pytestmark = pytest.mark.gpu
CRC = pytest.mark.parametrize("checksums", [True, False], ids=["crc", "nocrc"])
SCRATCH_ROUTE = 4096                      # a capacity above the 2048 nodes that the allocator keeps in LDS


@pytest.fixture(scope="module")
def ctx():
    return gridfour_amd.GvrsHipContext()


def dev_equals_host(ctx, image, records, tiles, status=None, flags=0, list_capacity=0):
    f = GvrsFileHip(image)
    u = f.update_begin()
    want = f.update_assemble(u, records, tiles, U.TIME, status, flags)
    cap = u.plan()[0]
    fst, n_bytes, buf = f.update_records_dev(ctx, u, records, tiles, U.TIME, status, flags, image_cap=cap, list_capacity=list_capacity)
    assert fst == _lib.OK and n_bytes == len(want)
    assert buf[:n_bytes] == want
    assert set(buf[max(n_bytes, len(image)):]) <= {0xA5}, "a byte behind the image was written"
    return want


@CRC
@pytest.mark.parametrize("name", sorted(U.SCENARIOS))
def test_records_form_equals_the_assembler(ctx, name, checksums):
    image, records, tiles, status, flags, _, _ = U.scenario(name, checksums)
    dev_equals_host(ctx, image, records, tiles, status, flags)


@pytest.mark.parametrize("name", ["exact fit", "a larger split", "free merges with both", "trailing node too small", "replace frees first"])
def test_records_form_in_scratch_equals_the_assembler(ctx, name):
    image, records, tiles, status, flags, _, _ = U.scenario(name)
    dev_equals_host(ctx, image, records, tiles, status, flags, list_capacity=SCRATCH_ROUTE)


@pytest.fixture(scope="module")
def chunk(tmp_path_factory):
    return read_chunk(tmp_path_factory)


@pytest.mark.parametrize("extended", [False, True], ids=["compact", "extended"])
@pytest.mark.parametrize("name,count", SEAMS, ids=[n for n, _ in SEAMS])
def test_directory_checksum_at_chunk_seams(ctx, chunk, name, count, extended):
    """The seam table of tests/dir_seams.py on the update's directory kernels: a grid of one row of n tiles, a file with
    tile 0 alone, and an update that writes tile 0 anew and the last tile, so that the new directory has n entries"""
    n = count(chunk, 8 if extended else 4)
    assert n >= 1
    image = U.make_file([("t", 0, 40)], grid=(2, 2 * n, 2, 2))
    got = dev_equals_host(ctx, image, *U.writes_of([(0, 48), (n - 1, 24)][:n]), flags=int(extended))
    td = struct.unpack_from("<q", got, 80)[0]
    (size,) = struct.unpack_from("<i", got, td - 8)
    assert struct.unpack_from("<iiii", got, td + 8) == (0, 0, 1, n) and got[td + 1] == int(extended)
    assert size == (8 + 8 + 16 + n * (8 if extended else 4) + 4 + 7) // 8 * 8
    assert struct.unpack_from("<I", got, td - 8 + size - 4)[0] == R.crc32c(got[td - 8:td - 8 + size - 4])    # (the Python loop, not the library's)


@CRC
def test_free_space_directory_cases(ctx, checksums):
    dev_equals_host(ctx, U.make_file(U.BASE, checksums), *U.writes_of([(3, 0)], checksums))
    layout = [("t", 0, 40), ("f", 64), ("t", 1, 48), ("t", 2, 24), ("t", 3, 56), ("t", 4, 24), ("t", 5, 40)]
    got = dev_equals_host(ctx, U.make_file(layout, checksums), *U.writes_of([(2, 0), (4, 0)], checksums))
    fs = struct.unpack_from("<q", got, 56)[0]
    assert struct.unpack_from("<ii", got, fs - 8) == (64, 3) and struct.unpack_from("<i", got, fs)[0] == 3     # consumed a node: roomier
    got = dev_equals_host(ctx, U.make_file([("t", 0, 40), ("t", 1, 48)], checksums), *U.writes_of([(7, 64)], checksums))
    assert struct.unpack_from("<q", got, 56)[0] == 0
    dev_equals_host(ctx, U.make_file(U.BASE, checksums, free_dir_slack=1), *U.writes_of([(50, 64)], checksums))


def test_a_second_update_and_a_file_with_metadata(ctx, golden_dir):
    image, records, tiles, *_ = U.scenario("replace frees first")
    once = dev_equals_host(ctx, image, records, tiles)
    dev_equals_host(ctx, once, *U.writes_of([(0, 0), (60, 32), (2, 0), (61, 400)], seed=5))
    # a reference file with a metadata directory: its four tiles rewritten with other sizes
    import os
    data = open(os.path.join(golden_dir, "ref_samples", "Sample05_IntComp.gvrs"), "rb").read()
    f = GvrsFileHip(data)
    assert f.info["metadata_dir_pos"] and f.info["codec_ids"]
    n_tiles = -(-f.grid[0] // f.grid[2]) * -(-f.grid[1] // f.grid[3])
    sizes = [0, 120, 24, 2048][:n_tiles]
    dev_equals_host(ctx, data, *U.writes_of(list(enumerate(sizes)), checksums=bool(f.info["checksum_enabled"])))


@pytest.mark.parametrize("route", [0, SCRATCH_ROUTE], ids=["lds", "scratch"])
@pytest.mark.parametrize("reverse", [False, True], ids=["append", "front"])
@pytest.mark.parametrize("n_nodes", [63, 64, 65, 128, 129])
def test_search_and_shift_seams(ctx, n_nodes, reverse, route):
    image, records, tiles = U.long_list(n_nodes, reverse)
    # the model first: the scenario really puts n_nodes nodes in front of the fitting one, each by an insert
    _, opened, _, writes, _ = U.model(image, records, tiles, n_tile_cols=U.BIG_TILE_COLS)
    assert len(opened) == 1
    assert [w[1] for w in writes[:n_nodes + 1]] == ["insert"] * (n_nodes + 1)
    assert writes[-1][:2] == ("alloc", "exact") and writes[-1][5] == n_nodes
    f = GvrsFileHip(image)
    u = f.update_begin()
    need = u.plan()[1]
    u.end()
    dev_equals_host(ctx, image, records, tiles, list_capacity=max(route, need) if route else 0)


def test_all_or_nothing_on_the_device(ctx):
    image, records, tiles, *_ = U.scenario("trailing node too small")
    f = GvrsFileHip(image)
    u = f.update_begin()
    want = f.update_assemble(u, records, tiles, U.TIME)
    for cap in (len(want) - 1, len(want) - 8, len(image)):
        fst, n_bytes, buf = f.update_records_dev(ctx, u, records, tiles, U.TIME, image_cap=cap)
        assert fst == _lib.ERR_CAPACITY and n_bytes == len(want)
        assert buf[:len(image)] == image and set(buf[len(image):]) <= {0xA5}
    fst, n_bytes, buf = f.update_records_dev(ctx, u, records, tiles, U.TIME, image_cap=len(want))
    assert fst == _lib.OK and buf[:n_bytes] == want and set(buf[n_bytes:]) <= {0xA5}


def test_device_refusals_change_nothing(ctx):
    image, records, tiles, *_ = U.scenario("exact fit")
    f = GvrsFileHip(image)
    u = f.update_begin()
    for recs, idx, code in (([records[0], records[0]], [50, 50], _lib.ERR_ARG), ([records[0]], [100], _lib.ERR_ARG),
                            ([records[0][:16]], [50], _lib.ERR_ARG)):
        fst, n_bytes, buf = f.update_records_dev(ctx, u, recs, idx, U.TIME)
        assert fst == code and n_bytes == 0 and buf[:len(image)] == image and set(buf[len(image):]) <= {0xA5}
    hurt = bytearray(image)
    struct.pack_into("<i", hurt, f.tile_position(2) - 8, 60)            # an old record whose size word is damaged
    u2 = f.update_begin(bytes(hurt))
    fst, n_bytes, buf = f.update_records_dev(ctx, u2, *U.writes_of([(2, 64)]), U.TIME)
    assert fst == _lib.ERR_FORMAT and buf[:len(hurt)] == bytes(hurt) and set(buf[len(hurt):]) <= {0xA5}


# ---- the block form in host memory ----
TILE, TILES = (4, 5), (5, 6)
BLOCK_GRID = (TILE[0] * TILES[0] - 1, TILE[1] * TILES[1] - 2) + TILE      # the last tile row and column are cut by the grid
RECTS = {"one tile": (4, 5, 4, 5), "several tiles": (4, 10, 8, 10), "partly covered on all sides": (2, 3, 9, 13), "whole grid": (0, 0) + BLOCK_GRID[:2]}


def block_spec(checksums):
    elements = [B.element("z", "int", fill=-9999), B.element("s", "short", fill=-1), B.element("c", "icf", fill=-2 ** 31, scale=4.0, offset=8.0)]
    return W.spec(BLOCK_GRID, elements, ["GvrsHuffman"], checksums, time_modified=5)


def rasters_of(seed, shape, hole=None):
    rng = np.random.default_rng(seed)
    z = rng.integers(-500, 500, shape).astype(np.int32)
    s = rng.integers(-300, 300, shape).astype(np.int16)
    c = (rng.integers(-4000, 4000, shape) / 4.0).astype(np.float32)      # (exact in the codes: scale 4, offset 8)
    if hole is not None:                                        # a tile's worth of fill: GF_DECLINED where it covers a tile
        r, q = hole
        z[r:r + TILE[0], q:q + TILE[1]] = -9999
        s[r:r + TILE[0], q:q + TILE[1]] = -1
        c[r:r + TILE[0], q:q + TILE[1]] = np.nan
    return [z, s, c]


@functools.lru_cache(maxsize=None)
def base(ctx, checksums):
    s = block_spec(checksums)
    rasters = rasters_of(1, BLOCK_GRID[:2])
    image, idx, status, _ = GvrsFileHip.write_image_host(ctx, W.lib_facts(s), rasters)
    assert (status == _lib.OK).all()
    return image, rasters


@pytest.mark.parametrize("name,checksums", [(n, True) for n in sorted(RECTS)] + [("partly covered on all sides", False)])
def test_block_form_in_host_memory(ctx, name, checksums):
    image, old = base(ctx, checksums)
    rect = RECTS[name]
    r0, c0, nr, nc = rect
    new = rasters_of(2, (nr, nc), hole=(8 - r0, 10 - c0) if name in ("several tiles", "whole grid") else None)
    f = GvrsFileHip(image)
    u = f.update_begin()
    out, idx, status, _ = f.update_image_host(ctx, u, rect, new, U.TIME)
    assert (status >= 0).all() and ((status == _lib.DECLINED).any() == (name in ("several tiles", "whole grid")))
    # placement and directories: the model, fed with the records the call laid
    g = GvrsFileHip(out)
    records = []
    for t, st in zip(idx, status):
        p = g.tile_position(int(t))
        assert (p == 0) == (st == _lib.DECLINED)
        records.append(out[p - 8:p - 8 + struct.unpack_from("<i", out, p - 8)[0]] if p else b"")
    want, _, final, _, _ = U.model(image, records, [int(t) for t in idx], n_tile_cols=TILES[1])
    assert out == want
    U.check_invariants(out, final, TILES[1])
    # the cells: the old raster with the rectangle replaced (NaN cells of the icf element are its fill)
    blocks, st, _ = g.read_block_dev(ctx, (0, 0) + BLOCK_GRID[:2])
    assert (st == _lib.OK).all()
    for e in range(3):
        expect = old[e].copy()
        expect[r0:r0 + nr, c0:c0 + nc] = new[e]
        assert np.array_equal(blocks[e], expect, equal_nan=(e == 2))


def update_hurt(ctx, image, rect, new):
    """the block form on a damaged image -> (return code, updated image, tile indices, statuses); the image equals the model's, fed
    with the records the call laid and its statuses"""
    f = GvrsFileHip(image)
    u = f.update_begin()
    rc, need, out, idx, status, _ = f.update_image_host(ctx, u, rect, new, U.TIME, return_code=True)
    assert need == len(out)
    g = GvrsFileHip(out)
    records = []
    for t, st in zip(idx, status):
        p = g.tile_position(int(t)) if st == _lib.OK else 0
        records.append(out[p - 8:p - 8 + struct.unpack_from("<i", out, p - 8)[0]] if p else b"")
    want, _, final, _, _ = U.model(image, records, [int(t) for t in idx], status=[int(s) for s in status], n_tile_cols=TILES[1])
    assert out == want
    return rc, out, idx.tolist(), status.tolist()


def test_damaged_old_records(ctx):
    image, old = base(ctx, True)
    f = GvrsFileHip(image)
    rect = RECTS["several tiles"]                               # tiles 8, 9, 14, 15, wholly covered
    new = rasters_of(3, rect[2:])
    # a wholly covered tile with a damaged old BODY is overwritten: its record is not decoded
    p8 = f.tile_position(8)
    hurt = bytearray(image)
    hurt[p8 + 12] ^= 0x55
    rc, out, idx, status = update_hurt(ctx, bytes(hurt), rect, new)
    assert rc == _lib.OK and idx == [8, 9, 14, 15] and status == [_lib.OK] * 4
    blocks, st, _ = GvrsFileHip(out).read_block_dev(ctx, rect)
    assert (st == _lib.OK).all() and all(np.array_equal(b, n) for b, n in zip(blocks, new))
    # one with a damaged SIZE WORD gets GF_ERR_FORMAT and stays, record and entry; the others are written
    p9 = f.tile_position(9)
    (size9,) = struct.unpack_from("<i", image, p9 - 8)
    hurt = bytearray(image)
    struct.pack_into("<i", hurt, p9 - 8, size9 - 4)
    rc, out, idx, status = update_hurt(ctx, bytes(hurt), rect, new)
    assert rc == _lib.ERR_FORMAT and status == [_lib.OK, _lib.ERR_FORMAT, _lib.OK, _lib.OK]
    g = GvrsFileHip(out)
    assert g.tile_position(9) == p9 and out[p9 - 8:p9 - 8 + size9] == bytes(hurt[p9 - 8:p9 - 8 + size9])
    blocks, st, _ = g.read_block_dev(ctx, (4, 10, 4, 5))
    assert (st == _lib.OK).all() and np.array_equal(blocks[0], new[0][:4, :5])
    # a partly covered tile whose old record fails keeps its status and stays
    rect = RECTS["partly covered on all sides"]                 # tile 0 is covered in part
    new = rasters_of(4, rect[2:])
    p0 = f.tile_position(0)
    (size0,) = struct.unpack_from("<i", image, p0 - 8)
    hurt = bytearray(image)
    hurt[p0 + 12] ^= 0x55                                       # the record's checksum no longer holds
    rc, out, idx, status = update_hurt(ctx, bytes(hurt), rect, new)
    assert idx[0] == 0 and status[0] < 0 and rc == status[0] and all(s == _lib.OK for s in status[1:])
    assert GvrsFileHip(out).tile_position(0) == p0 and out[p0 - 8:p0 - 8 + size0] == bytes(hurt[p0 - 8:p0 - 8 + size0])


# ---- the block form in device memory ----
@pytest.mark.parametrize("name,checksums", [(n, True) for n in sorted(RECTS)] + [("partly covered on all sides", False), ("several tiles", False)])
def test_device_block_form_equals_the_host_form(ctx, name, checksums):
    image, old = base(ctx, checksums)
    rect = RECTS[name]
    r0, c0, nr, nc = rect
    new = rasters_of(2, (nr, nc), hole=(8 - r0, 10 - c0) if name in ("several tiles", "whole grid") else None)
    f = GvrsFileHip(image)
    u = f.update_begin()
    want, h_idx, h_status, h_used = f.update_image_host(ctx, u, rect, new, U.TIME)
    cap = u.plan(rect)[0]
    fst, n_bytes, buf, idx, status, used = f.update_image(ctx, u, rect, new, U.TIME, image_cap=cap, raw=True)
    assert fst == _lib.OK and n_bytes == len(want)
    assert np.array_equal(idx, h_idx) and np.array_equal(status, h_status) and np.array_equal(used, h_used)
    assert buf[:n_bytes] == want and set(buf[max(n_bytes, len(image)):]) <= {0xA5}
    blocks, st, _ = GvrsFileHip(buf[:n_bytes]).read_block_dev(ctx, (0, 0) + BLOCK_GRID[:2])
    assert (st == _lib.OK).all()
    for e in range(3):
        expect = old[e].copy()
        expect[r0:r0 + nr, c0:c0 + nc] = new[e]
        assert np.array_equal(blocks[e], expect, equal_nan=(e == 2))
    # one byte too little room (where the file grows at all): status and size as stated, the image as it was uploaded
    if len(want) > len(image):
        fst, need, buf, _, _, _ = f.update_image(ctx, u, rect, new, U.TIME, image_cap=len(want) - 1, raw=True)
        assert fst == _lib.ERR_CAPACITY and need == len(want) and buf[:len(image)] == image and set(buf[len(image):]) <= {0xA5}


def device_equals_host_on(ctx, image, rect, new):
    f = GvrsFileHip(image)
    u = f.update_begin()
    rc, need, want, h_idx, h_status, _ = f.update_image_host(ctx, u, rect, new, U.TIME, return_code=True)
    fst, n_bytes, buf, idx, status, _ = f.update_image(ctx, u, rect, new, U.TIME, raw=True)
    assert fst == _lib.OK and n_bytes == need == len(want) and buf[:n_bytes] == want
    assert np.array_equal(idx, h_idx) and np.array_equal(status, h_status)
    return buf[:n_bytes], status.tolist()


def test_damaged_old_records_on_the_device(ctx):
    image, old = base(ctx, True)
    f = GvrsFileHip(image)
    for rect in (RECTS["several tiles"], (4, 10, 8, 9)):       # tile-aligned, and the same tiles with 9 and 15 covered in part
        new = rasters_of(3, rect[2:])
        p8, p9 = f.tile_position(8), f.tile_position(9)
        hurt = bytearray(image)
        hurt[p8 + 12] ^= 0x55                                   # a wholly covered tile with a damaged body: overwritten
        out, status = device_equals_host_on(ctx, bytes(hurt), rect, new)
        assert status == [_lib.OK] * 4
        (size9,) = struct.unpack_from("<i", image, p9 - 8)
        hurt = bytearray(image)
        struct.pack_into("<i", hurt, p9 - 8, size9 - 4)         # a damaged size word: GF_ERR_FORMAT, and the tile stays
        out, status = device_equals_host_on(ctx, bytes(hurt), rect, new)
        assert status == [_lib.OK, _lib.ERR_FORMAT, _lib.OK, _lib.OK]
        assert GvrsFileHip(out).tile_position(9) == p9 and out[p9 - 8:p9 - 8 + size9] == bytes(hurt[p9 - 8:p9 - 8 + size9])
    rect = RECTS["partly covered on all sides"]                 # tile 0 is covered in part; its old record's checksum fails
    new = rasters_of(4, rect[2:])
    p0 = f.tile_position(0)
    (size0,) = struct.unpack_from("<i", image, p0 - 8)
    hurt = bytearray(image)
    hurt[p0 + 12] ^= 0x55
    out, status = device_equals_host_on(ctx, bytes(hurt), rect, new)
    assert status[0] < 0 and all(s == _lib.OK for s in status[1:])
    assert GvrsFileHip(out).tile_position(0) == p0 and out[p0 - 8:p0 - 8 + size0] == bytes(hurt[p0 - 8:p0 - 8 + size0])


def test_records_form_and_aligned_block_form_only_enqueue(ctx):
    """Behind a backlog of memsets on the context's stream each call must return while the backlog still runs: an event recorded
    behind the call is not ready.  (Each call follows a synchronisation: a call waits only for an EARLIER call's copies to leave the
    context's page-locked buffer.)  The results are then the host forms'."""
    import ctypes as C
    import caller_stream as CS
    from gridfour_amd.codec import _DeviceScope, _blob_of, _ptr, lib
    S = CS.Stream(ctx.stream)
    image, records, tiles, *_ = U.scenario("replace frees first")
    f = GvrsFileHip(image)
    u = f.update_begin()
    want = f.update_assemble(u, records, tiles, U.TIME)
    cap = u.plan()[0]
    blob, offsets = _blob_of(records)
    idx = np.ascontiguousarray(tiles, np.int32)
    b_image, b_old = base(ctx, True)
    g = GvrsFileHip(b_image)
    gu = g.update_begin()
    rect = np.ascontiguousarray(RECTS["several tiles"], np.int32)
    new = rasters_of(5, tuple(rect[2:]))
    b_want, _, _, _ = g.update_image_host(ctx, gu, rect, new, U.TIME)
    b_cap = gu.plan(rect)[0]
    with _DeviceScope(ctx) as s:
        backlog = s.alloc(1 << 30)
        buf = np.full(cap, 0xA5, np.uint8)
        buf[:len(image)] = np.frombuffer(image, np.uint8)
        d_image, d_blob, d_off, d_idx = s.upload(buf), s.upload(blob, slack=16), s.upload(offsets, slack=16), s.upload(idx, slack=16)
        d_bytes, d_fst = s.alloc(16, fill=0x7f), s.alloc(16, fill=0x7f)
        b_buf = np.full(b_cap, 0xA5, np.uint8)
        b_buf[:len(b_image)] = np.frombuffer(b_image, np.uint8)
        d_bimage = s.upload(b_buf)
        d_blk = [s.upload(np.ascontiguousarray(b), slack=16) for b in new]
        d_tidx, d_st, d_used = s.alloc(4 * 4 + 16, fill=0x7f), s.alloc(4 * 4 + 16, fill=0x7f), s.alloc(3 * 4 + 16, fill=0)

        def records_call():
            return lib().gf_file_update_records_dev(ctx.handle, u.handle, d_image.ptr, cap, d_blob.ptr, d_off.ptr, d_idx.ptr, None, idx.size,
                                                    int(offsets[-1]), U.TIME, 0, 0, d_bytes.ptr, d_fst.ptr)

        def block_call():
            return lib().gf_file_update_block_elems_dev(ctx.handle, gu.handle, _ptr(rect), s.ptrs(d_blk), 0, U.TIME, d_bimage.ptr, b_cap,
                                                        d_bytes.ptr, d_fst.ptr, d_tidx.ptr, d_st.ptr, d_used.ptr)

        for call, d_img, old_image, expect in ((records_call, d_image, image, want), (block_call, d_bimage, b_image, b_want)):
            assert call() == _lib.OK                              # warm-up: module load, the context's buffers
            ctx.synchronize()
            d_img.upload(np.frombuffer(old_image, np.uint8))
            ctx.synchronize()
            for _ in range(64):
                S.memset(backlog.ptr, 0, 1 << 30)
            assert call() == _lib.OK
            e = S.event()
            S.record(e)
            ready = CS.hip().hipEventQuery(e)
            ctx.synchronize()
            assert ready == CS.HIP_NOT_READY, "the call returned only when the stream had drained (or the backlog was too short)"
            assert int(d_fst.download(np.int32, 1)[0]) == _lib.OK
            assert d_img.download(np.uint8, len(expect)).tobytes() == expect
    for e in S._events:
        CS.hip().hipEventDestroy(e)
