"""Blocks read from GVRS file images (gf_file_read_block_elems[_dev] behind GvrsFileHip, k_file_locate) and GF_CODEC_LSOP08 as a list
kind: the reference's fifteen sample files read as files against the records calls fed by hand, images of the test-only writer
gvrs_file_build.py -- records shuffled between junk, absent tiles, a directory over a sub-rectangle, compact and extended
entries -- against numpy, damaged directory entries and record heads one at a time, and LSOP08 packings under a codec list."""
import os
import struct

import numpy as np
import pytest

import gridfour_amd
from gridfour_amd import _lib

import gvrs_file_build as B
from gvrs_walk import walk_records
from test_file_open import FACTS, SAMPLES, sample_path

pytestmark = pytest.mark.gpu
INT_MIN = -2 ** 31
OK, ERR_FORMAT, ERR_BOUNDS = _lib.OK, _lib.ERR_FORMAT, _lib.ERR_BOUNDS
PLAIN = (0, 1, 2, 3, 9, 10, 11, 12)                         # every cell is row * gridCols + col - 1


@pytest.fixture(scope="module")
def ctx():
    return gridfour_amd.GvrsHipContext()


def both_forms(f, ctx, rect, verify=True, image=None):
    """the rectangle through the device form and the host form: they must agree; returns the device form's answer"""
    dev = f.read_block_dev(ctx, rect, verify, image=image)
    host = f.read_block(ctx, rect, verify, image=image)
    for a, b in zip(dev[0], host[0]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert dev[1].tolist() == host[1].tolist() and dev[2].tolist() == host[2].tolist()
    return dev


def by_hand(ctx, k, golden_dir, rect):
    """the sample through CodecMasterHip.read_block: the records the chain walk finds, the facts handed over by hand"""
    grid, _, elems, ids, _, _, _, _ = FACTS[k]
    data = open(sample_path(golden_dir, k), "rb").read()
    records = [data[pos:pos + size] for pos, size, rtype, _ in walk_records(data) if rtype == 2]
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.uint64)
    kinds = {"GvrsHuffman": 1, "GvrsDeflate": 2, "GvrsFloat": 0, "LSOP12": 4}
    master = gridfour_amd.CodecMasterHip(codec_list=[kinds[i] for i in ids], context=ctx)
    specs = [e[1] if e[1] != "icf" else ("icf", e[3], e[4], e[2], e[5]) for e in elems]
    return master.read_block(grid[2], grid[3], grid[:2], rect, np.frombuffer(b"".join(records), np.uint8), offsets, specs,
                             verify_checksums=bool(FACTS[k][1]))


@pytest.mark.parametrize("k", range(15))
def test_samples_whole_grid(ctx, golden_dir, k):
    grid = FACTS[k][0]
    rect = (0, 0, grid[0], grid[1])
    f = gridfour_amd.GvrsFileHip(sample_path(golden_dir, k))
    blocks, status, present = both_forms(f, ctx, rect)
    want, want_status = by_hand(ctx, k, golden_dir, rect)
    assert not status.any() and not want_status.any() and present.tolist() == [1] * len(FACTS[k][7])
    for a, b in zip(blocks, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if k in PLAIN:
        rows, cols = np.meshgrid(np.arange(grid[0]), np.arange(grid[1]), indexing="ij")
        assert np.array_equal(blocks[0], (rows * grid[1] + cols - 1).astype(blocks[0].dtype))


@pytest.mark.parametrize("k,rect", [(5, (49, 48, 3, 5)), (9, (7, 6, 3, 4)), (8, (4, 3, 3, 4)), (6, (99, 0, 1, 100))])
def test_samples_seams(ctx, golden_dir, k, rect):
    f = gridfour_amd.GvrsFileHip(sample_path(golden_dir, k))
    blocks, status, present = both_forms(f, ctx, rect)
    want, _ = by_hand(ctx, k, golden_dir, rect)
    whole, _ = by_hand(ctx, k, golden_dir, (0, 0) + FACTS[k][0][:2])
    assert not status.any() and present.all()
    for a, b, w in zip(blocks, want, whole):
        assert a.tobytes() == b.tobytes()
        assert a.tobytes() == np.ascontiguousarray(w[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]]).tobytes()


# ---- 299 tiles: past a 256-lane workgroup and several waves of k_file_locate ----
GRID299 = (45, 37, 2, 3)


def image299(extended):
    """(image, positions of the named tiles, the grid as the file delivers it).  Records shuffled with junk between them, a third of
    the tiles without a record, the directory over tile rows 2..20 and columns 1..11 only: tiles outside it are absent too."""
    nr, nc, tr, tc = GRID299
    n_tile_rows, n_tile_cols = 23, 13
    rng = np.random.default_rng(299)
    rows, cols = np.meshgrid(np.arange(n_tile_rows * tr), np.arange(n_tile_cols * tc), indexing="ij")
    cells = (rows * 1000 + cols).astype(np.int32)            # (tiles reach beyond the grid: their cells there are never delivered)
    held = [t for t in range(299) if rng.integers(0, 3) != 0]
    records = {}
    for t in held:
        r, c = divmod(t, n_tile_cols)
        records[t] = B.standard_record(t, [cells[r * tr:(r + 1) * tr, c * tc:(c + 1) * tc]])
    order = list(rng.permutation(held))

    def between(k):
        kind = k % 4
        if kind == 0:
            return b""
        if kind == 1:
            return B.other_record(B.RECORD_METADATA, 40 + k % 64, seed=k)
        return rng.integers(0, 256, 8 * (1 + k % 5), dtype=np.uint8).tobytes()
    image, named = B.build_image(GRID299, [B.element("z", "int")], records, order=order, between=between, dir_rect=(2, 1, 19, 11), extended=extended)
    want = np.full((n_tile_rows * tr, n_tile_cols * tc), INT_MIN, np.int32)
    for t in named:
        r, c = divmod(t, n_tile_cols)
        want[r * tr:(r + 1) * tr, c * tc:(c + 1) * tc] = cells[r * tr:(r + 1) * tr, c * tc:(c + 1) * tc]
    return image, named, want[:nr, :nc]


@pytest.fixture(scope="module", params=[False, True], ids=["compact", "extended"])
def file299(request):
    image, named, want = image299(request.param)
    return gridfour_amd.GvrsFileHip(image), named, want


@pytest.mark.parametrize("rect", [(0, 0, 45, 37), (3, 2, 40, 33), (5, 4, 1, 1), (38, 30, 7, 7)])
def test_299_tiles(ctx, file299, rect):
    f, named, want = file299
    assert 120 < len(named) < 160 and f.info["dir_extended"] in (0, 1)
    blocks, status, present = both_forms(f, ctx, rect)
    r0, c0, nr, nc = rect
    assert np.array_equal(blocks[0], want[r0:r0 + nr, c0:c0 + nc])
    tiles = [r * 13 + c for r in range(r0 // 2, (r0 + nr - 1) // 2 + 1) for c in range(c0 // 3, (c0 + nc - 1) // 3 + 1)]
    assert status.shape == (1, len(tiles)) and not status.any()          # an absent tile reads as fill with status 0
    assert present.tolist() == [int(t in named) for t in tiles]
    if rect == (0, 0, 45, 37):
        assert len(tiles) == 299 and 0 < present.sum() < 299 and (blocks[0] == INT_MIN).any() and (blocks[0] != INT_MIN).any()
        assert [f.tile_position(t) for t in range(299)] == [named.get(t, 0) for t in range(299)]


# ---- compressed records of the samples laid anew ----
@pytest.mark.parametrize("k", [5, 6])
def test_compressed_records_relaid(ctx, golden_dir, k):
    grid, _, elems, ids, _, _, _, positions = FACTS[k]
    data = open(sample_path(golden_dir, k), "rb").read()
    records = {t: data[p - 8:p - 8 + struct.unpack_from("<i", data, p - 8)[0]] for t, p in enumerate(positions)}
    kind = elems[0][1]
    image, named = B.build_image(grid, [B.element(elems[0][0], kind)], records, codec_ids=ids, order=[3, 2, 1, 0], extended=True,
                                 between=lambda k: B.other_record(B.RECORD_METADATA, 24, seed=k))
    f, sample = gridfour_amd.GvrsFileHip(image), gridfour_amd.GvrsFileHip(sample_path(golden_dir, k))
    assert f.info["dir_extended"] == 1 and [named[t] for t in range(4)] != positions
    rect = (0, 0, grid[0], grid[1])
    got, want = both_forms(f, ctx, rect), both_forms(sample, ctx, rect)
    assert got[0][0].tobytes() == want[0][0].tobytes() and not got[1].any() and got[2].tolist() == [1, 1, 1, 1]


# ---- damage, one case each: only that tile's status changes, its cells are fill, every other tile is intact ----
GRID_D = (7, 5, 3, 2)                                         # 3 x 3 tiles


def image_d(extended, **kw):
    rows, cols = np.meshgrid(np.arange(9), np.arange(6), indexing="ij")
    cells = (rows * 100 + cols + 1).astype(np.int32)
    records = {t: B.standard_record(t, [cells[(t // 3) * 3:(t // 3) * 3 + 3, (t % 3) * 2:(t % 3) * 2 + 2]]) for t in range(9)}
    image, named = B.build_image(GRID_D, [B.element("z", "int")], records, order=[4, 8, 0, 6, 2, 7, 1, 5, 3], extended=extended,
                                 between=lambda k: B.other_record(B.RECORD_METADATA, 16, seed=k) if k % 2 else b"", **kw)
    return image, named, cells[:7, :5]


def check_damage(ctx, extended, damage, tile, want_status, verify=True, filled=None):
    """damage(image, positions, f) -> the damaged image, read through the handle of the sound one; filled: the tile's cells read as fill
    (default: where its status is not GF_OK)"""
    image, named, want = image_d(extended)
    f = gridfour_amd.GvrsFileHip(image)
    sound = both_forms(f, ctx, (0, 0, 7, 5), verify)
    assert np.array_equal(sound[0][0], want) and not sound[1].any() and sound[2].all()
    bad = damage(image, named, f)
    assert len(bad) == len(image)
    blocks, status, present = both_forms(f, ctx, (0, 0, 7, 5), verify, image=bad)
    want_st = np.zeros((1, 9), np.int32)
    want_st[0, tile] = want_status
    assert status.tolist() == want_st.tolist()
    want = want.copy()
    if want_status != OK if filled is None else filled:
        r, c = divmod(tile, 3)
        want[r * 3:r * 3 + 3, c * 2:c * 2 + 2] = INT_MIN
    assert np.array_equal(blocks[0], want)
    return present


def put(image, at, raw):
    return image[:at] + raw + image[at + len(raw):]


def entry(value, extended):
    def damage(image, named, f):
        at, w = B.entry_offset(image, f.info, 4)
        v = value(image, named, f) if callable(value) else value
        return put(image, at, struct.pack("<q", v) if extended else struct.pack("<I", v))
    return damage


def test_damage_compact_entry_16_gib(ctx):
    present = check_damage(ctx, False, entry(0x80000000, False), 4, ERR_BOUNDS)      # a position of 16 GiB in an image of a few KB
    assert present.all()


@pytest.mark.parametrize("name,value", [
    ("negative", -8),
    ("most negative", -2 ** 63),
    ("no multiple of 8", lambda im, named, f: named[4] + 4),
    ("below the content", lambda im, named, f: f.info["content_pos"]),
    ("within 12 bytes of the end", lambda im, named, f: (len(im) - 8) // 8 * 8),
    ("the end itself", lambda im, named, f: len(im) // 8 * 8),
    ("far behind the end", 1 << 40),
], ids=lambda x: x if isinstance(x, str) else "")
def test_damage_extended_entry(ctx, name, value):
    check_damage(ctx, True, entry(value, True), 4, ERR_BOUNDS)


def test_damage_entry_cleared(ctx):
    for extended in (False, True):                           # no record: fill, status 0, not present
        present = check_damage(ctx, extended, entry(0, extended), 4, OK, filled=True)
        assert present.tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1]


@pytest.mark.parametrize("extended", [False, True], ids=["compact", "extended"])
def test_last_entry_behind_the_image_end(ctx, extended):
    """the directory is the image's last record: an image cut inside, or in front of, its last entry refuses that tile alone"""
    rows, cols = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    cells = (rows * 100 + cols + 1).astype(np.int32)
    records = {t: B.standard_record(t, [cells[(t // 2) * 8:(t // 2) * 8 + 8, (t % 2) * 8:(t % 2) * 8 + 8]]) for t in range(4)}
    image, _ = B.build_image((16, 16, 8, 8), [B.element("z", "int")], records, extended=extended)
    f = gridfour_amd.GvrsFileHip(image)
    at, w = B.entry_offset(image, f.info, 3)
    # entry 3 is the directory's last and the directory the image's last record: only its padding and checksum lie behind
    assert f.info["dir_n_rows"] * f.info["dir_n_cols"] == 4 and len(image) - (at + w) == 8
    want = cells.copy()
    want[8:, 8:] = INT_MIN
    for cut in (at + w - 1, at):
        blocks, status, present = both_forms(f, ctx, (0, 0, 16, 16), image=image[:cut])
        assert status.tolist() == [[OK, OK, OK, ERR_BOUNDS]] and present.tolist() == [1, 1, 1, 0]
        assert np.array_equal(blocks[0], want)


@pytest.mark.parametrize("size", [0, 12, 16, 124, 1 << 20, -8])
def test_damage_size_word(ctx, size):
    check_damage(ctx, True, lambda im, named, f: put(im, named[4] - 8, struct.pack("<i", size)), 4, ERR_BOUNDS)


def test_damage_type_byte(ctx):
    check_damage(ctx, False, lambda im, named, f: put(im, named[4] - 4, b"\x03"), 4, ERR_FORMAT)


def test_damage_tile_index_word(ctx):
    check_damage(ctx, False, lambda im, named, f: B.refresh_record_crc(put(im, named[4], struct.pack("<i", 5)), named[4]), 4, ERR_FORMAT)


def test_damage_two_entries_name_one_record(ctx):
    for extended in (False, True):
        check_damage(ctx, extended, entry(lambda im, named, f: named[5] if extended else named[5] // 8, extended), 4, ERR_FORMAT)


def test_damage_record_crc(ctx):
    def damage(im, named, f):
        (size,) = struct.unpack_from("<i", im, named[4] - 8)
        return put(im, named[4] - 8 + size - 4, bytes([im[named[4] - 8 + size - 4] ^ 0x10]))
    check_damage(ctx, True, damage, 4, ERR_FORMAT, verify=True)
    check_damage(ctx, True, damage, 4, OK, verify=False)


def test_rectangle_outside_the_grid_and_unknown_codec(ctx):
    image, _, _ = image_d(False)
    f = gridfour_amd.GvrsFileHip(image)
    for rect in ((0, 0, 8, 5), (-1, 0, 2, 2), (0, 4, 1, 2), (0, 0, 0, 1)):
        for read in (f.read_block, f.read_block_dev):
            with pytest.raises(gridfour_amd.GvrsHipError) as e:
                read(ctx, rect)
            assert e.value.status == _lib.ERR_ARG
    image, _, _ = image_d(False, codec_ids=["GvrsHuffman", "SomethingElse"])
    f = gridfour_amd.GvrsFileHip(image)
    for read in (f.read_block, f.read_block_dev):
        with pytest.raises(gridfour_amd.GvrsHipError) as e:
            read(ctx, (0, 0, 7, 5))
        assert e.value.status == _lib.ERR_UNSUPPORTED


# ---- GF_CODEC_LSOP08 as a list kind ----
def terrain(n, nr, nc, seed):
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(nr), np.arange(nc), indexing="ij")
    out = []
    for t in range(n):
        a, b, c = rng.uniform(0.05, 0.4, 3)
        z = 800 * np.sin(a * x + t) * np.cos(b * y) + 40 * np.sin(c * (x + y)) + rng.integers(-3, 4, (nr, nc))
        out.append(np.rint(z).astype(np.int32))
    return np.stack(out)


@pytest.mark.parametrize("nr,nc", [(4, 4), (24, 17)])
def test_lsop08_file_form(ctx, nr, nc):
    """tiles packed by gf_lsop08_encode_batch_i32 under index 0, framed under the id LSOP08, read back"""
    n_tile_rows, n_tile_cols = 3, 2
    tiles = terrain(6, nr, nc, seed=nr)
    packings, _, st = gridfour_amd.LsCodec08Hip(context=ctx).encode_batch(0, nr, nc, tiles)
    std = 4 * nr * nc
    records, n_packed = {}, 0
    for t in range(6):
        p = packings[t]
        if p is not None and st[t] == OK and len(p) != std:           # (what the encoder declines goes in standard form, as a writer lays it)
            records[t] = B.frame_record(t, [p])
            n_packed += 1
        else:
            records[t] = B.standard_record(t, [tiles[t]])
    if (nr, nc) == (24, 17):
        assert n_packed == 6
    grid = (n_tile_rows * nr - 1, n_tile_cols * nc - 2, nr, nc)
    image, _ = B.build_image(grid, [B.element("z", "int")], records, codec_ids=["LSOP08"], order=[5, 0, 3, 1, 4, 2])
    f = gridfour_amd.GvrsFileHip(image)
    assert f.info["codecs"] == [gridfour_amd.CODEC_LSOP08]
    blocks, status, present = both_forms(f, ctx, (0, 0, grid[0], grid[1]))
    want = np.block([[tiles[r * n_tile_cols + c] for c in range(n_tile_cols)] for r in range(n_tile_rows)])[:grid[0], :grid[1]]
    assert not status.any() and present.all() and np.array_equal(blocks[0], want)


def test_lsop08_mixed_list(ctx):
    """gf_codec_master_decode_batch_i32_dev over a shuffled batch under [HUFFMAN, LSOP08, LSOP12] against the three decoders alone"""
    nr, nc = 24, 17
    tiles = terrain(9, nr, nc, seed=8)
    codecs = [gridfour_amd.CodecHuffmanHip(context=ctx), gridfour_amd.LsCodec08Hip(context=ctx), gridfour_amd.LsCodecHip(context=ctx)]
    packs, alone = [], []
    for k, codec in enumerate(codecs):
        p, _, st = codec.encode_batch(k, nr, nc, tiles[3 * k:3 * k + 3])
        assert not st.any() and all(x[0] == k for x in p)
        v, dst = codec.decode_batch(nr, nc, p)
        assert not dst.any() and np.array_equal(v.reshape(3, nr, nc), tiles[3 * k:3 * k + 3])
        packs += p
        alone += list(v)
    order = [4, 0, 8, 3, 7, 1, 5, 2, 6]
    master = gridfour_amd.CodecMasterHip(codec_list=[gridfour_amd.CODEC_HUFFMAN, gridfour_amd.CODEC_LSOP08, gridfour_amd.CODEC_LSOP12], context=ctx)
    values, status = master.decode_batch_dev(nr, nc, [packs[j] for j in order])
    assert not status.any()
    for got, j in zip(values, order):
        assert np.array_equal(got, alone[j])
    host_values, host_status = master.decode_batch(nr, nc, [packs[j] for j in order])            # the host codec master takes the kind too
    assert not host_status.any() and np.array_equal(host_values, values)
    # a packing that names index 1 under [HUFFMAN, LSOP12] still fails as before: LSOP12 refuses an LSOP08 container
    old = gridfour_amd.CodecMasterHip(codec_list=[gridfour_amd.CODEC_HUFFMAN, gridfour_amd.CODEC_LSOP12], context=ctx)
    _, st = old.decode_batch_dev(nr, nc, [packs[3], packs[0], packs[4]])
    assert st.tolist() == [ERR_FORMAT, OK, ERR_FORMAT]
    # ... and a kind outside the list's range is still an argument error
    with pytest.raises(gridfour_amd.GvrsHipError) as e:
        gridfour_amd.CodecMasterHip(codec_list=[1, 9], context=ctx).decode_batch_dev(nr, nc, [packs[0]])
    assert e.value.status == _lib.ERR_ARG


def test_lsop08_records_written_by_the_host_form(ctx):
    """the host record writer takes the kind, the device record writer answers GF_ERR_UNSUPPORTED as for LSOP12"""
    nr, nc = 24, 17
    tiles = terrain(4, nr, nc, seed=3)
    master = gridfour_amd.CodecMasterHip(codec_list=[gridfour_amd.CODEC_LSOP08], context=ctx)
    records, used = master.tile_records_elems(nr, nc, [0, 1, 2, 3], [tiles], ["int"])
    assert used.tolist() == [[0, 0, 0, 0]]
    image, _ = B.build_image((2 * nr, 2 * nc, nr, nc), [B.element("z", "int")], dict(enumerate(records)), codec_ids=["LSOP08"], extended=True)
    blocks, status, _ = both_forms(gridfour_amd.GvrsFileHip(image), ctx, (0, 0, 2 * nr, 2 * nc))
    assert not status.any() and np.array_equal(blocks[0], np.block([[tiles[0], tiles[1]], [tiles[2], tiles[3]]]))
    with pytest.raises(gridfour_amd.GvrsHipError) as e:
        master.tile_records_elems_dev(nr, nc, [0, 1, 2, 3], [tiles], ["int"])
    assert e.value.status == _lib.ERR_UNSUPPORTED
