"""GVRS file images written on the GPU (gf_file_write_block_elems_dev and its host form).  Every image is held to three things: it
opens and reads back what went in (gf_file_open, gf_file_read_block_elems_dev); it equals gf_file_assemble fed with the records
gf_block_write_elems_dev gives for the same blocks, in row-major order; and it equals the image tests/gvrs_file_write_ref.py
builds in Python around those records.  Shapes are the smallest at which a path can go wrong: grids that are no multiple of the
tile, bounding rectangles that shrink, directories of one entry and at the seams of the checksum's chunks, capacities inside
every part of the image."""
import functools
import struct

import numpy as np
import pytest

import gridfour_amd
from gridfour_amd import GvrsFileHip, GvrsHipError, FILE_DIR_EXTENDED
from gridfour_amd import _lib

import gvrs_file_build as B
import gvrs_file_write_ref as W
from dir_seams import SEAMS, read_chunk

pytestmark = pytest.mark.gpu
F32 = np.float32
INT_MIN = -2 ** 31
HUFFMAN, CANON = "GvrsHuffman", "GvrsCanonicalHuffman"
STANDARD = ["GvrsHuffman", "GvrsDeflate", "GvrsFloat"]
META = [("GvrsJavaCodecs", 0, 6, b"GvrsHuffman, org.gridfour.compress.CodecHuffman\n", "Class paths for Java compressors"),
        ("empty", 7, 0, b"", ""), ("Copyright", 1, 6, bytes(range(40)), "of the data"),
        # a front too long for the finishing kernel's arguments (3,072 bytes): it is copied to the image before the kernels run
        ("long", 2, 1, np.random.default_rng(4).integers(0, 256, 5001, dtype=np.uint8).tobytes(), "a long record")]


@pytest.fixture(scope="module")
def ctx():
    return gridfour_amd.GvrsHipContext()


@functools.lru_cache(maxsize=None)
def _master(ctx, kinds):
    return gridfour_amd.CodecMasterHip(codec_list=list(kinds), context=ctx)


def element(kind, **kw):
    if kind == "icf":                       # a power of two as the scale: the header's float range is exact in any arithmetic
        return B.element("z_icf", "icf", vmin=INT_MIN + 1, vmax=2 ** 31 - 2, scale=4.0, offset=-3.0, label="coded", unit="m", continuous=True, **kw)
    return B.element("z_" + kind, kind, label=kind.upper(), description="an element of type " + kind, **kw)


def make_spec(tile, tiles, kinds, ids, short_by=(1, 2), **kw):
    """A grid of tiles[0] x tiles[1] tiles of tile[0] x tile[1] cells, short_by cells short of a multiple of the tile"""
    grid = (tiles[0] * tile[0] - short_by[0], tiles[1] * tile[1] - short_by[1], tile[0], tile[1])
    elements = kw.pop("elements", None) or [element(k) for k in kinds]
    return W.spec(grid, elements, ids, uuid=bytes(range(16)), time_modified=0x18f0a1b2c3d, product_label="written on the device", **kw)


def raster(el, grid, seed=0):
    """smooth data inside every range, no cell equal to a fill"""
    r, c = np.meshgrid(np.arange(grid[0]), np.arange(grid[1]), indexing="ij")
    if el["kind"] == "int":
        return (1000 + 3 * r + 2 * c + (r * c) // 7 + 17 * seed).astype(np.int32)
    if el["kind"] == "short":
        return (-200 + 2 * r + c + (r + 2 * c) // 5 - 3 * seed).astype(np.int16)
    if el["kind"] == "float":
        return (0.5 * r + 0.25 * c + 1.0 + seed).astype(F32)
    return (0.25 * (r * 3 + c) + 0.5 * seed).astype(F32)          # multiples of 1 / scale: the codes give them back exactly


def fill_of(el):
    return {"int": np.int32, "short": np.int16}[el["kind"]](el["fill"]) if el["kind"] in ("int", "short") else F32(el["fill"] if el["kind"] == "float" else el["fill_f"])


def crop(arrays, rect):
    r0, c0, nr, nc = rect
    return [np.ascontiguousarray(a[r0:r0 + nr, c0:c0 + nc]) for a in arrays]


def tiles_of(s, rect):
    """the tile indices a rect touches, row-major"""
    g = s["grid"]
    n_tile_cols = -(-g[1] // g[3])
    return [tr * n_tile_cols + tc for tr in range(rect[0] // g[2], (rect[0] + rect[2] - 1) // g[2] + 1)
            for tc in range(rect[1] // g[3], (rect[1] + rect[3] - 1) // g[3] + 1)]


def read_back(ctx, s, image, rasters, rect, absent=()):
    """The image opens, every status is GF_OK, and the whole grid reads as the rasters inside rect and fill elsewhere; absent: tiles
    inside rect that have no record and read as fill"""
    g = s["grid"]
    f = GvrsFileHip(image)
    blocks, status, _ = f.read_block_dev(ctx, (0, 0, g[0], g[1]))
    assert (status == _lib.OK).all(), status
    n_tile_cols = -(-g[1] // g[3])
    for el, got, src in zip(s["elements"], blocks, rasters):
        want = np.full((g[0], g[1]), fill_of(el))
        want[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]] = src[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]]
        for t in absent:
            tr, tc = t // n_tile_cols, t % n_tile_cols
            want[tr * g[2]:(tr + 1) * g[2], tc * g[3]:(tc + 1) * g[3]] = fill_of(el)
        np.testing.assert_array_equal(got, want, err_msg=el["name"])
    info = f.info
    f.close()
    return info


def write_and_compare(ctx, s, rasters, rect, flags=0):
    """The device form's image == gf_file_assemble over gf_block_write_elems_dev's records == the Python writer's; returns (image,
    tile indices, statuses)"""
    g = s["grid"]
    facts = W.lib_facts(s)
    image, idx, status, used = GvrsFileHip.write_image(ctx, facts, crop(rasters, rect), rect, flags=flags)
    elems, fills = W.elems_of(s)
    ranges = [None if el["kind"] == "icf" else (el["vmin"], el["vmax"]) for el in s["elements"]]
    master = _master(ctx, tuple(W.KINDS[c] for c in s["codec_ids"]))
    b_idx, recs, b_used, b_status = master.write_block_dev(g[2], g[3], g[:2], rect, crop(rasters, rect), elems, fills=fills, ranges=ranges,
                                                           checksums=s["checksums"])
    assert np.array_equal(idx, b_idx) and np.array_equal(status, b_status) and np.array_equal(used, b_used)
    assert idx.tolist() == tiles_of(s, rect)
    assert image == GvrsFileHip.assemble(facts, recs, b_idx, flags=flags), "the device form differs from the assembler"
    assert image == W.ref_image(s, list(zip(b_idx.tolist(), recs)), extended=bool(flags)), "the device form differs from the Python writer"
    return image, idx, status


# ---------------------------------------------------------------- 4. round trip

ROUND = [((4, 5), (2, 2), ["int", "short", "icf"], [HUFFMAN]),
         ((3, 8), (5, 7), ["int", "short", "icf"], [CANON]),
         ((4, 5), (3, 4), ["short", "int"], [HUFFMAN, CANON]),
         ((3, 8), (2, 3), ["icf", "int", "short"], []),
         ((4, 5), (5, 7), ["int", "float", "short", "icf"], []),
         ((3, 8), (2, 2), ["float"], [])]


@pytest.mark.parametrize("tile,tiles,kinds,ids", ROUND, ids=["%dx%d-%dx%d-%s-%d" % (t + n + ("".join(k[0] for k in ks), len(i))) for t, n, ks, i in ROUND])
def test_round_trip(ctx, tile, tiles, kinds, ids):
    s = make_spec(tile, tiles, kinds, ids, metadata=META[:1])
    g = s["grid"]
    rasters = [raster(el, g) for el in s["elements"]]
    for rect in ((0, 0, g[0], g[1]), (1, 2, g[0] - 2, g[1] - 3)):
        image, idx, status, _ = GvrsFileHip.write_image(ctx, W.lib_facts(s), crop(rasters, rect), rect)
        assert (status == _lib.OK).all() and idx.tolist() == tiles_of(s, rect)
        info = read_back(ctx, s, image, rasters, rect)
        assert (info["dir_row0"], info["dir_col0"], info["dir_n_rows"], info["dir_n_cols"]) == (0, 0) + tuple(tiles)
        assert info["codec_ids"] == ids and info["metadata_dir_pos"] != 0 and info["freespace_dir_pos"] == 0


# ---------------------------------------------------------------- 5. image equality

EQUAL = [(0, True, 0), (1, True, 0), (3, True, 0), (3, False, 0), (1, True, FILE_DIR_EXTENDED), (0, False, FILE_DIR_EXTENDED), (4, True, 0),
         (4, False, FILE_DIR_EXTENDED)]


@pytest.mark.parametrize("n_meta,checksums,flags", EQUAL, ids=["meta%d-crc%d-ext%d" % e for e in EQUAL])
def test_image_equals_the_assembler_and_the_python_writer(ctx, n_meta, checksums, flags):
    s = make_spec((4, 5), (3, 4), ["int", "short", "icf"], [HUFFMAN, CANON], checksums=checksums, metadata=META[:n_meta])
    g = s["grid"]
    rasters = [raster(el, g, seed=n_meta) for el in s["elements"]]
    rect = (2, 1, g[0] - 3, g[1] - 2)
    image, _, status = write_and_compare(ctx, s, rasters, rect, flags)
    assert (status == _lib.OK).all()
    info = read_back(ctx, s, image, rasters, rect)
    assert info["dir_extended"] == int(bool(flags)) and (info["metadata_dir_pos"] != 0) == bool(n_meta)
    s4 = make_spec((3, 8), (2, 3), ["int", "float", "short", "icf"], [], checksums=checksums, metadata=META[:n_meta])
    r4 = [raster(el, s4["grid"], seed=3) for el in s4["elements"]]
    write_and_compare(ctx, s4, r4, (0, 0) + s4["grid"][:2], flags)


# ---------------------------------------------------------------- 6. the bounding rectangle

def bounding_spec():
    return make_spec((4, 5), (4, 5), [], [HUFFMAN], metadata=META[:1],
                     elements=[element("int", vmin=-1000, vmax=5000), element("short")])


def with_fill(s, rasters, tiles):
    """the rasters with the cells of `tiles` set to the elements' fills"""
    g = s["grid"]
    n_tile_cols = -(-g[1] // g[3])
    out = [a.copy() for a in rasters]
    for t in tiles:
        tr, tc = t // n_tile_cols, t % n_tile_cols
        for el, a in zip(s["elements"], out):
            a[tr * g[2]:(tr + 1) * g[2], tc * g[3]:(tc + 1) * g[3]] = fill_of(el)
    return out


def tile_rect(s, tr0, tc0, ntr, ntc):
    g = s["grid"]
    return (tr0 * g[2], tc0 * g[3], min(ntr * g[2], g[0] - tr0 * g[2]), min(ntc * g[3], g[1] - tc0 * g[3]))


BOUNDING = {
    "corner tile": (lambda s: (s["grid"][0] - 2, s["grid"][1] - 2, 2, 2), [], (3, 4, 1, 1)),
    "inner row": (lambda s: tile_rect(s, 1, 0, 1, 5), [], (1, 0, 1, 5)),
    "outer row and column all fill": (lambda s: tile_rect(s, 0, 0, 3, 4), [0, 1, 2, 3, 5, 10], (1, 1, 2, 3)),
    "L": (lambda s: tile_rect(s, 1, 1, 3, 3), [7, 8, 12, 13], (1, 1, 3, 3)),
    "all declined": (lambda s: tile_rect(s, 0, 1, 2, 2), [1, 2, 6, 7], (0, 0, 0, 0)),
}


@pytest.mark.parametrize("case", list(BOUNDING))
def test_bounding_rectangle(ctx, case):
    s = bounding_spec()
    rect_of, declined, want_dir = BOUNDING[case]
    rect = rect_of(s)
    rasters = with_fill(s, [raster(el, s["grid"]) for el in s["elements"]], declined)
    image, idx, status = write_and_compare(ctx, s, rasters, rect)
    assert [int(t) for t, st in zip(idx, status) if st == _lib.DECLINED] == declined
    assert all(st in (_lib.OK, _lib.DECLINED) for st in status)
    info = read_back(ctx, s, image, rasters, rect)
    assert (info["dir_row0"], info["dir_col0"], info["dir_n_rows"], info["dir_n_cols"]) == want_dir
    f = GvrsFileHip(image)
    assert [t for t in range(20) if f.tile_position(t)] == [int(t) for t, st in zip(idx, status) if st == _lib.OK]
    if case == "all declined":
        (size,) = struct.unpack_from("<i", image, info["tile_dir_pos"] - 8)
        assert size == 40 and len(image) == info["tile_dir_pos"] - 8 + 40


def test_a_tile_out_of_range_gets_no_record_and_the_file_reads(ctx):
    s = bounding_spec()
    g = s["grid"]
    rasters = [raster(el, g) for el in s["elements"]]
    rasters[0][5, 7] = 99999                                  # tile 6, inside the box, above the INT element's vmax of 5000
    rect = tile_rect(s, 0, 0, 3, 3)
    image, idx, status = write_and_compare(ctx, s, rasters, rect)
    assert status.tolist() == [_lib.ERR_BOUNDS if t == 6 else _lib.OK for t in idx]
    info = read_back(ctx, s, image, rasters, rect, absent=[6])
    assert (info["dir_row0"], info["dir_col0"], info["dir_n_rows"], info["dir_n_cols"]) == (0, 0, 3, 3)
    assert GvrsFileHip(image).tile_position(6) == 0


# ---------------------------------------------------------------- 7. the seams of the checksum's chunks

@pytest.fixture(scope="module")
def chunk(tmp_path_factory):
    return read_chunk(tmp_path_factory)


@pytest.mark.parametrize("extended", [False, True], ids=["compact", "extended"])
@pytest.mark.parametrize("name,count", SEAMS, ids=[n for n, _ in SEAMS])
def test_directory_checksum_at_chunk_seams(ctx, chunk, name, count, extended):
    n = count(chunk, 8 if extended else 4)
    assert n >= 1
    s = W.spec((2, 2 * n, 2, 2), [element("int")], [], uuid=bytes(16), time_modified=5)
    rasters = [raster(s["elements"][0], s["grid"])]
    image, idx, status = write_and_compare(ctx, s, rasters, (0, 0, 2, 2 * n), FILE_DIR_EXTENDED if extended else 0)
    assert (status == _lib.OK).all() and idx.size == n
    f = GvrsFileHip(image)
    i = f.info
    assert (i["dir_row0"], i["dir_col0"], i["dir_n_rows"], i["dir_n_cols"], i["dir_extended"]) == (0, 0, 1, n, int(extended))
    at = i["tile_dir_pos"] - 8
    (size,) = struct.unpack_from("<i", image, at)
    assert at + size == len(image) and size == (8 + 8 + 16 + n * (8 if extended else 4) + 4 + 7) // 8 * 8
    assert struct.unpack_from("<I", image, at + size - 4)[0] == B.crc32c(image[at:at + size - 4])
    blocks, st, _ = f.read_block_dev(ctx, (0, 2 * n - 2, 2, 2))                    # the last tile, through the last entry
    assert (st == _lib.OK).all() and np.array_equal(blocks[0], rasters[0][:, -2:])


# ---------------------------------------------------------------- 8. capacity

@pytest.mark.parametrize("n_meta", [2, 4], ids=["front in the arguments", "front copied"])
def test_capacity(ctx, n_meta):
    s = make_spec((4, 5), (2, 3), ["int", "short"], [HUFFMAN], metadata=META[:n_meta])
    g = s["grid"]
    rasters = [raster(el, g) for el in s["elements"]]
    rect = (0, 0, g[0], g[1])
    facts = W.lib_facts(s)
    whole, idx, status, _ = GvrsFileHip.write_image(ctx, facts, rasters, rect)
    need = len(whole)
    f = GvrsFileHip(whole)
    meta_dir, third = f.info["metadata_dir_pos"] - 8, f.tile_position(2) - 8
    first, most = facts.plan(rect)
    assert first == f.tile_position(0) - 8 and need <= most
    extents = [(f.tile_position(t) - 8, f.tile_position(t) - 8 + struct.unpack_from("<i", whole, f.tile_position(t) - 8)[0]) for t in range(6)]
    assert extents[0][0] == first and extents[-1][1] == meta_dir and all(a[1] == b[0] for a, b in zip(extents, extents[1:]))
    f.close()
    for cap in (need, need + 24, need - 8, meta_dir + 8, third + 16, first, first - 24, 200, 16, 8):
        fst, n_bytes, buf, c_idx, c_status, _ = GvrsFileHip.write_image(ctx, facts, rasters, rect, image_cap=cap, raw=True)
        assert n_bytes == need, cap
        assert buf.size == cap + 64 and (buf[cap:] == 0xA5).all(), "a byte at or behind image_cap was written (cap %d)" % cap
        assert np.array_equal(c_idx, idx) and np.array_equal(c_status, status)
        if cap >= need:
            assert fst == _lib.OK and buf[:need].tobytes() == whole and (buf[need:] == 0xA5).all()
            continue
        assert fst == _lib.ERR_CAPACITY, cap
        assert not buf[:min(cap, 16)].any(), "the file head of an image that does not fit is not zero (cap %d)" % cap
        with pytest.raises(GvrsHipError):
            GvrsFileHip(buf[:cap].tobytes())
        for start, end in extents:                            # a record that fits is whole, one that does not is not begun
            if end <= cap:
                assert buf[start:end].tobytes() == whole[start:end], (cap, start)
            else:
                assert (buf[max(start, 16):min(end, cap)] == 0xA5).all(), (cap, start)
    with pytest.raises(GvrsHipError) as e:
        GvrsFileHip.write_image(ctx, facts, rasters, rect, image_cap=need - 8)
    assert e.value.status == _lib.ERR_CAPACITY


# ---------------------------------------------------------------- 9. the host form

@pytest.mark.parametrize("ids", [[HUFFMAN], [], [HUFFMAN, CANON]], ids=["huffman", "none", "both"])
def test_host_form_equals_the_device_form(ctx, ids):
    s = make_spec((4, 5), (3, 4), ["int", "short", "icf"], ids, metadata=META[:3])
    g = s["grid"]
    rasters = with_fill(s, [raster(el, g) for el in s["elements"]], [0, 5])
    rect = (0, 0, g[0] - 1, g[1] - 2)
    facts = W.lib_facts(s)
    for flags in (0, FILE_DIR_EXTENDED):
        d_image, d_idx, d_status, d_used = GvrsFileHip.write_image(ctx, facts, crop(rasters, rect), rect, flags=flags)
        h_image, h_idx, h_status, h_used = GvrsFileHip.write_image_host(ctx, facts, crop(rasters, rect), rect, flags=flags)
        assert h_image == d_image and np.array_equal(h_idx, d_idx) and np.array_equal(h_status, d_status) and np.array_equal(h_used, d_used)
        assert [int(t) for t, st in zip(h_idx, h_status) if st == _lib.DECLINED] == [0, 5]
        # the records fit and the tile directory does not; then not even the records
        for cap in (len(h_image) - 8, GvrsFileHip(h_image).tile_position(6)):
            rc, need, part, _, _, _ = GvrsFileHip.write_image_host(ctx, facts, crop(rasters, rect), rect, flags=flags, image_cap=cap, return_code=True)
            assert rc == _lib.ERR_CAPACITY and need == len(h_image), (flags, cap)


def test_host_form_with_the_standard_list_reads_back(ctx):
    s = make_spec((8, 10), (3, 3), ["int", "short", "float", "icf"], STANDARD, metadata=META[:1])
    g = s["grid"]
    rasters = [raster(el, g) for el in s["elements"]]
    rect = (3, 1, g[0] - 4, g[1] - 3)
    facts = W.lib_facts(s)
    image, idx, status, used = GvrsFileHip.write_image_host(ctx, facts, crop(rasters, rect), rect)
    assert (status == _lib.OK).all() and idx.tolist() == tiles_of(s, rect)
    info = read_back(ctx, s, image, rasters, rect)
    assert info["codec_ids"] == STANDARD and (used != 255).any()
    # the device form takes no list with CodecDeflate: refused from the arguments alone
    with pytest.raises(GvrsHipError) as e:
        GvrsFileHip.write_image(ctx, facts, crop(rasters, rect), rect)
    assert e.value.status == _lib.ERR_UNSUPPORTED
