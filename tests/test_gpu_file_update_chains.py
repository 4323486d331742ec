"""The in-place update on the GPU past the seams of its launches (the inputs: tests/file_update_chains.py, which
tests/test_file_update_chains_inputs.py shows to do what they claim and holds to the model on the host).
gf_file_update_records_dev is held to gf_file_update_assemble byte for byte, with the guard behind the image intact: on lists of
64 .. 130 nodes at open with one erase, merge, split, insert or end-of-file allocation at a node index on either side of the
64-node turns, in both routes of the list (LDS and scratch); on seeded chains of updates fed from the device's OWN bytes, whose last
image the GPU inspector then passes; on files whose final list takes k_update_fill's grid-stride loop into a second and a third
turn; on 131 records with one refusal planted past the first turn of the judging loop; on 257 .. 399 records with empty ones on
the seams of k_update_copy's workgroups.  One block-form update of 81 tiles has a damaged old record at slot 70."""
import struct

import numpy as np
import pytest

import gridfour_amd
from gridfour_amd import GvrsFileHip, _lib
from gridfour_amd.codec import _DeviceScope

import file_update_cases as U
import file_update_chains as K
import gvrs_file_build as B
import gvrs_file_write_ref as W

pytestmark = pytest.mark.gpu
ROUTES = pytest.mark.parametrize("route", ["lds", "scratch"])
SCRATCH_ROUTE = 4096                      # a capacity above the 2048 nodes that the allocator keeps in LDS


@pytest.fixture(scope="module")
def ctx():
    return gridfour_amd.GvrsHipContext()


def dev_equals_host(ctx, image, records, tiles, status=None, route="lds", name=None):
    """-> the DEVICE's image: status, size and bytes the assembler's, nothing written behind it"""
    f = GvrsFileHip(image)
    u = f.update_begin()
    want = f.update_assemble(u, records, tiles, U.TIME, status)
    cap, plan = u.plan()
    fst, n_bytes, buf = f.update_records_dev(ctx, u, records, tiles, U.TIME, status, image_cap=cap,
                                             list_capacity=max(SCRATCH_ROUTE, plan) if route == "scratch" else 0)
    u.end()
    assert fst == _lib.OK and n_bytes == len(want), name
    assert buf[:n_bytes] == want, name
    assert set(buf[max(n_bytes, len(image)):]) <= {0xA5}, f"a byte behind the image was written: {name}"
    return buf[:n_bytes]


@ROUTES
@pytest.mark.parametrize("n", K.N_NODES)
def test_one_list_event_on_a_long_list(ctx, n, route):
    for name, (image, records, tiles, _) in K.directed(n).items():
        dev_equals_host(ctx, image, records, tiles, route=route, name=name)


@ROUTES
@pytest.mark.parametrize("seed,n_rounds,checksums", K.CHAINS, ids=[f"seed{c[0]}" for c in K.CHAINS])
def test_chain_fed_from_the_device(ctx, seed, n_rounds, checksums, route):
    image = K.chain_start(seed, checksums)
    for rnd in range(1, n_rounds + 1):
        records, tiles, status = K.chain_round(seed, rnd, image, checksums)
        before = image
        image = dev_equals_host(ctx, image, records, tiles, status, route, name=rnd)      # the next round opens the device's bytes
    final = U.model(before, records, tiles, status, n_tile_cols=U.BIG_TILE_COLS)[2]
    f = GvrsFileHip(image)
    want, got = f.inspect(), f.inspect_dev(ctx)
    assert got.report() == want.report() and got.bad_tiles == want.bad_tiles and got.records == want.records and got.guards_intact
    assert got.passed and got.complete and got.termination_pos == len(image)
    assert [(r[0], r[1]) for r in got.records if r[2] == 0] == final


@pytest.mark.parametrize("several", [False, True], ids=["one node", "several nodes"])
@pytest.mark.parametrize("name", sorted(K.FILLS))
def test_fill_past_its_first_turn(ctx, name, several):
    image, records, tiles = K.fill_case(K.FILLS[name], several)
    got = dev_equals_host(ctx, image, records, tiles, name=name)
    fs = struct.unpack_from("<q", got, 56)[0]
    (n,) = struct.unpack_from("<i", got, fs)
    nodes = [struct.unpack_from("<qi", got, fs + 4 + 12 * k) for k in range(n)]
    assert sum(z for _, z in nodes) == K.FILLS[name]
    for p, z in nodes:                                             # each node, read for itself: head, zeros, the head's checksum
        assert got[p:p + z] == U.free_node(z), (p, z)


def records_dev_raw(ctx, image, blob, offsets, tiles):
    """gf_file_update_records_dev with the caller's own offsets -> (file status, size, the buffer), as update_records_dev calls it"""
    f = GvrsFileHip(image)
    u = f.update_begin()
    cap = u.plan()[0]
    buf = np.full(cap + 64, 0xA5, np.uint8)
    buf[:len(image)] = np.frombuffer(image, np.uint8)
    with _DeviceScope(ctx) as s:
        d_image, d_blob, d_off, d_idx = s.upload(buf), s.upload(blob, slack=16), s.upload(offsets, slack=16), s.upload(tiles, slack=16)
        d_bytes, d_fst = s.alloc(16, fill=0x7f), s.alloc(16, fill=0x7f)
        s.run("gf_file_update_records_dev", ctx.handle, u.handle, d_image.ptr, cap, d_blob.ptr, d_off.ptr, d_idx.ptr, None, tiles.size,
              blob.size - 16, U.TIME, 0, 0, d_bytes.ptr, d_fst.ptr)
        out = int(d_fst.download(np.int32, 1)[0]), int(d_bytes.download(np.uint64, 1)[0]), d_image.download(np.uint8, cap + 64).tobytes()
    u.end()
    return out


def test_refusals_past_the_first_turn_of_the_judge(ctx):
    image, blob, cases = K.judge_cases()
    rc, want, need = K.assemble_raw(image, blob, *cases["valid"])
    fst, n_bytes, buf = records_dev_raw(ctx, image, blob, *cases["valid"])
    assert rc == fst == _lib.OK and n_bytes == need and buf[:n_bytes] == want[:need] and set(buf[n_bytes:]) <= {0xA5}
    for name, (offsets, tiles) in cases.items():
        if name != "valid":
            assert K.assemble_raw(image, blob, offsets, tiles)[0] == _lib.ERR_ARG, name
            fst, n_bytes, buf = records_dev_raw(ctx, image, blob, offsets, tiles)
            assert fst == _lib.ERR_ARG and n_bytes == 0, name
            assert buf[:len(image)] == image and set(buf[len(image):]) <= {0xA5}, name


@pytest.mark.parametrize("n", K.BATCHES)
def test_patch_and_copy_past_one_workgroup(ctx, n):
    image, records, tiles = K.batch(n)
    got = dev_equals_host(ctx, image, records, tiles, name=n)
    g = GvrsFileHip(got)
    for r, t in zip(records, tiles):                               # every record where its entry names it, every freed tile without one
        p = g.tile_position(t)
        assert (got[p - 8:p - 8 + len(r)] == r) if r else p == 0, t


def test_block_form_with_a_damaged_record_past_the_first_turn(ctx):
    """81 tiles in the rectangle, the old record at slot 70 with a damaged size word: k_update_alloc gives that tile its verdict,
    resets its own and goes on, behind the 64 records of the judging loop's first turn.  The device form equals the host form."""
    import test_gpu_file_update as T
    grid = (9 * T.TILE[0], 9 * T.TILE[1]) + T.TILE
    elements = [B.element("z", "int", fill=-9999), B.element("s", "short", fill=-1), B.element("c", "icf", fill=-2 ** 31, scale=4.0, offset=8.0)]
    image, _, status, _ = GvrsFileHip.write_image_host(ctx, W.lib_facts(W.spec(grid, elements, ["GvrsHuffman"], True, time_modified=5)),
                                                       T.rasters_of(1, grid[:2]))
    assert (status == _lib.OK).all() and status.size == 81
    f = GvrsFileHip(image)
    p70 = f.tile_position(70)
    (size70,) = struct.unpack_from("<i", image, p70 - 8)
    hurt = bytearray(image)
    struct.pack_into("<i", hurt, p70 - 8, size70 - 4)
    for rect in ((0, 0) + grid[:2], (2, 3, grid[0] - 2, grid[1] - 3)):       # tile-aligned, and with the first tile row and column covered in part
        out, status = T.device_equals_host_on(ctx, bytes(hurt), rect, T.rasters_of(3, rect[2:]))
        assert len(status) == 81 and status[70] == _lib.ERR_FORMAT and all(s == _lib.OK for k, s in enumerate(status) if k != 70)
        g = GvrsFileHip(out)
        assert g.tile_position(70) == p70 and out[p70 - 8:p70 - 8 + size70] == bytes(hurt[p70 - 8:p70 - 8 + size70])
