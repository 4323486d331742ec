"""Tile records and mixed-codec packings decoded where they lie in device memory (gf_tile_record_decode_batch_dev,
gf_codec_master_decode_batch_i32_dev): the reference's own sample files, and record by record the host entry points
gf_tile_record_decode_batch / gf_codec_master_decode_batch_i32 on the same bytes -- statuses, tile indices and the values of every
GF_OK tile must be identical."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import damage as D
from gvrs_walk import walk_records
from test_gpu_records import _crc32c, _ramp
from tilegen import make_tile

pytestmark = pytest.mark.gpu
NULL = -2**31
HUFFMAN, DEFLATE, NONE, CANON, LSOP = 1, 2, 0, 3, 4
LIST5 = (HUFFMAN, DEFLATE, NONE, CANON, LSOP)            # codec indices 0, 1, (2: no integer codec), 3, 4
NR, NC = 40, 60


def _p(a):
    return C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def ctx():
    import gridfour_amd
    return gridfour_amd.GvrsHipContext()


@pytest.fixture(scope="module")
def master5(ctx):
    import gridfour_amd
    return gridfour_amd.CodecMasterHip(codec_list=LIST5, context=ctx)


def _crc(b):
    from gridfour_amd._lib import lib
    return lib().gf_crc32c(C.c_char_p(bytes(b)), len(b))


def _frame(index, element, crc=True):
    """RecordManager's framing of one element: size, type 2, index, n, the bytes, zero padding, CRC-32C (or 0)"""
    n = len(element)
    size = (8 + n + 12 + 7) // 8 * 8
    r = bytearray(size)
    struct.pack_into("<iB3xii", r, 0, size, 2, index, n)
    r[16:16 + n] = element
    if crc:
        struct.pack_into("<I", r, size - 4, _crc(r[:size - 4]))
    return bytes(r)


def _frame_elems(index, elements, crc=True, size=None):
    """RecordManager's framing of a tile of several elements: size, type 2, index, per element [n][bytes], padding, CRC-32C"""
    body = b"".join(struct.pack("<i", len(el)) + el for el in elements)
    if size is None:
        size = (4 + len(body) + 12 + 7) // 8 * 8
    r = bytearray(max(size, 12 + len(body)))
    struct.pack_into("<iB3xi", r, 0, size, 2, index)
    r[12:12 + len(body)] = body
    r = r[:size]
    if crc:
        struct.pack_into("<I", r, size - 4, _crc(r[:size - 4]))
    return bytes(r)


def _refresh_crc(r):
    size = len(r)
    r = bytearray(r)
    struct.pack_into("<I", r, size - 4, _crc(r[:size - 4]))
    return bytes(r)


def _concat(records):
    offsets = np.zeros(len(records) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in records])
    return np.frombuffer(b"".join(records) + b"\0" * 16, np.uint8)[:int(offsets[-1])], offsets


def _shifted(records, seed):
    """record i at a byte offset = i mod 8 with filler in front of it and behind the last one (a record's span runs through the filler)"""
    rng = np.random.default_rng(seed)
    parts, offsets, pos = [], [], 0
    for i, rec in enumerate(records):
        gap = int(rng.integers(1, 24))
        gap += (i % 8 - (pos + gap)) % 8
        parts.append(bytes(rng.integers(1, 256, gap, dtype=np.uint8)))
        pos += gap
        offsets.append(pos)
        parts.append(rec)
        pos += len(rec)
    parts.append(bytes(rng.integers(1, 256, 13, dtype=np.uint8)))
    offsets.append(pos + 13)
    return np.frombuffer(b"".join(parts), np.uint8), np.array(offsets, np.uint64)


def _host_records(master, nr, nc, blob, offsets, element, verify):
    """gf_tile_record_decode_batch on a blob and an offsets array as given"""
    from gridfour_amd._lib import check, lib
    short = element == "short"
    nt = len(offsets) - 1
    blob = np.concatenate([np.asarray(blob, np.uint8), np.zeros(16, np.uint8)])
    offsets = np.ascontiguousarray(offsets, np.uint64)
    out = np.zeros((nt, nr * nc), np.int16 if short else np.int32)
    idx = np.full(nt, -1, np.int32)
    status = np.zeros(nt, np.int32)
    codecs = master.codecs if master.codecs.size else np.zeros(1, np.int32)
    check(lib().gf_tile_record_decode_batch(master.ctx.handle, _p(codecs), master.codecs.size, int(short), nr, nc, nt, _p(blob),
                                            _p(offsets), int(bool(verify)), _p(idx), _p(out), _p(status)), "gf_tile_record_decode_batch")
    return idx, out, status


def _same_as_host(master, nr, nc, blob, offsets, element, verify, what=""):
    """the device form against the host call on the same bytes; returns the (common) result"""
    hi, hv, hs = _host_records(master, nr, nc, blob, offsets, element, verify)
    di, dv, ds = master.record_blob_dev(nr, nc, blob, offsets, element=element, verify_checksums=verify)
    assert np.array_equal(ds, hs), (what, verify, ds.tolist(), hs.tolist())
    assert np.array_equal(di, hi), (what, verify, di.tolist(), hi.tolist())
    ok = hs == 0
    assert np.array_equal(dv[ok], hv[ok]), (what, verify)
    return hi, hv, hs


# ---------------------------------------------------------------- 1. the reference's own bytes

SAMPLES = [
    # file, element, tile size, grid columns, codec list (None = the standard list)
    ("Sample05_IntComp.gvrs", "int", 50, 100, None),
    ("Sample04_ShortComp.gvrs", "short", 50, 100, None),
    ("Sample01_IntNoComp.gvrs", "int", 5, 10, []),
    ("Sample00_ShortNoComp.gvrs", "short", 5, 10, []),
]


@pytest.mark.parametrize("name,element,tile,grid_cols,codecs", SAMPLES, ids=[c[0][:8] for c in SAMPLES])
def test_reference_sample_records(golden_dir, ctx, name, element, tile, grid_cols, codecs):
    """the four tile records of a sample file, uploaded as they lie in the file (with whatever lies between them), checksums
    verified: the file's tile indices and the ramp the reference wrote"""
    import gridfour_amd
    master = gridfour_amd.CodecMasterHip(context=ctx) if codecs is None else gridfour_amd.CodecMasterHip(codec_list=codecs, context=ctx)
    with open(os.path.join(golden_dir, "ref_samples", name), "rb") as f:
        data = f.read()
    spans = [(pos, size, struct.unpack_from("<i", content, 0)[0]) for pos, size, rtype, content in walk_records(data) if rtype == 2]
    assert len(spans) == 4
    lo = min(p for p, _, _ in spans) & ~3
    hi = max(p + s for p, s, _ in spans)
    blob = np.frombuffer(data[lo:hi], np.uint8)
    want_idx = [i for _, _, i in spans]
    want = np.stack([_ramp(i, grid_cols, tile) for i in want_idx]).astype(np.int16 if element == "short" else np.int32)
    # (the device form takes one offsets array: a record's span runs to the next record's start, as file order has it)
    order = np.argsort([p for p, _, _ in spans])
    offsets = np.array([spans[k][0] - lo for k in order] + [hi - lo], np.uint64)
    idx, got, st = master.record_blob_dev(tile, tile, blob, offsets, element=element, verify_checksums=True)
    assert (st == 0).all(), st
    assert list(idx) == [want_idx[k] for k in order]
    assert np.array_equal(got, want[order])


# ---------------------------------------------------------------- 2. every codec in one batch

def _source_tiles(element):
    """24 tiles of 40 x 60: five per integer codec, four for the standard form; a block of nulls in each codec's third"""
    per_codec = ["smooth", "noise8", "steps", "noise16", "sparse_big"]
    tiles, plan = [], []
    for slot in (0, 1, 3, 4):
        for j, kind in enumerate(per_codec):
            t = make_tile(kind, NR, NC, seed=11 * slot + j).copy()
            if j == 2:
                t.reshape(NR, NC)[10:20, 5:50] = NULL
            tiles.append(t)
            plan.append(slot)
    for j, kind in enumerate(["noise32", "extremes", "smooth", "ramp"]):
        tiles.append(make_tile(kind, NR, NC, seed=90 + j).copy())
        plan.append(None)
    tiles = np.stack(tiles).astype(np.int32)
    if element == "short":
        tiles = np.where(tiles == NULL, NULL, np.clip(tiles, -32767, 32767)).astype(np.int32)
    return tiles, plan


def _mixed(ctx, element):
    """(records, packings, plan): every tile encoded by ONE chosen codec's host encoder and framed here"""
    import gridfour_amd
    tiles, plan = _source_tiles(element)
    enc = {0: gridfour_amd.CodecHuffmanHip(context=ctx), 1: gridfour_amd.CodecDeflateHip(context=ctx),
           3: gridfour_amd.CodecCanonHuffmanHip(context=ctx), 4: gridfour_amd.LsCodecHip(context=ctx)}
    packs = [None] * len(tiles)
    for slot, codec in enc.items():
        members = [i for i, s in enumerate(plan) if s == slot]
        got = codec.encode_batch(slot, NR, NC, tiles[members])[0]
        for i, pk in zip(members, got):
            packs[i] = pk                                    # (None: the encoder declined; the tile takes the standard form)
    std = NR * NC * (2 if element == "short" else 4)
    records, elements = [], []
    for i, pk in enumerate(packs):
        if pk is not None and len(pk) < std:
            el = pk
        elif element == "short":
            el = np.where(tiles[i] == NULL, -32768, tiles[i]).astype("<i2").tobytes()
        else:
            el = tiles[i].astype("<i4").tobytes()
        elements.append(el)
        records.append(_frame(1000 + 7 * i, el))
    order = np.random.default_rng(5).permutation(len(records))
    return [records[k] for k in order], [elements[k] for k in order], tiles[order]


@pytest.fixture(scope="module")
def mixed_int(ctx):
    return _mixed(ctx, "int")


@pytest.fixture(scope="module")
def mixed_short(ctx):
    return _mixed(ctx, "short")


def _owners(elements, std):
    own = {}
    for el in elements:
        k = "std" if len(el) == std else el[0]
        own[k] = own.get(k, 0) + 1
    return own


@pytest.mark.parametrize("element", ["int", "short"])
def test_every_codec_in_one_batch(master5, mixed_int, mixed_short, element):
    records, elements, tiles = mixed_int if element == "int" else mixed_short
    own = _owners(elements, NR * NC * (2 if element == "short" else 4))
    assert all(own.get(k, 0) >= 3 for k in (0, 1, 3, 4, "std")), own          # no codec absent, the standard form present
    blob, offsets = _concat(records)
    for verify in (True, False):
        idx, vals, st = _same_as_host(master5, NR, NC, blob, offsets, element, verify)
        assert (st == 0).all()
        want = np.where(tiles == NULL, -32768, tiles).astype(np.int16) if element == "short" else tiles
        assert np.array_equal(vals, want)


def test_mixed_packings_without_framing(master5, mixed_int):
    records, elements, tiles = mixed_int
    packs = [el for el in elements if len(el) != NR * NC * 4]
    keep = [i for i, el in enumerate(elements) if len(el) != NR * NC * 4]
    hv, hs = master5.decode_batch(NR, NC, packs)
    dv, ds = master5.decode_batch_dev(NR, NC, packs)
    assert (hs == 0).all() and np.array_equal(ds, hs) and np.array_equal(dv, hv) and np.array_equal(dv, tiles[keep])
    # an empty packing, one that names the entry without an integer codec, one outside the list
    odd = packs[:3] + [b"", b"\x02" + packs[0][1:], b"\x05" + packs[0][1:]] + packs[3:6]
    hv, hs = master5.decode_batch(NR, NC, odd)
    dv, ds = master5.decode_batch_dev(NR, NC, odd)
    assert np.array_equal(ds, hs) and list(hs[3:6]) == [-1, -1, -1] and np.array_equal(dv[hs == 0], hv[hs == 0])
    # the documented difference: a packing that ends behind blob_bytes is GF_ERR_BOUNDS, its neighbours are unaffected
    blob = np.frombuffer(b"".join(packs[:3]), np.uint8)
    lengths = np.array([len(p) for p in packs[:3]], np.uint32)
    offsets = np.array([0, len(packs[0]), len(packs[0]) + len(packs[1])], np.uint64)
    offsets[1], lengths[1] = blob.size - 4, 5
    dv, ds = master5.packing_blob_dev(NR, NC, blob, offsets, lengths)
    assert list(ds) == [0, -2, 0] and np.array_equal(dv[[0, 2]], tiles[keep][[0, 2]])


# ---------------------------------------------------------------- 3. framing and checksum verdicts

def _put32(r, at, v):
    r = bytearray(r)
    struct.pack_into("<I", r, at, v & 0xFFFFFFFF)
    return bytes(r)


def _flip(r, byte, bit):
    r = bytearray(r)
    r[byte] ^= 1 << bit
    return bytes(r)


def test_framing_and_checksum_verdicts(ctx, master5, mixed_int):
    import gridfour_amd
    records, elements, _ = mixed_int
    good = records[:12]
    std = NR * NC * 4
    # the victim: a packed record with padding in front of its checksum
    v = next(i for i, r in enumerate(good) if len(elements[i]) != std and len(r) - 4 - 16 - len(elements[i]) > 0)
    r = good[v]
    size, n = len(r), len(elements[v])

    def batch(record):
        return good[:v] + [record] + good[v + 1:]

    # a single flipped bit: caught by the checksum wherever it is; without verification the host call decides
    for what, rec in (("header bit", _flip(r, 9, 2)), ("packing bit", _flip(r, 16 + n // 2, 5)), ("padding bit", _flip(r, 16 + n, 0))):
        blob, offsets = _concat(batch(rec))
        _, _, st = _same_as_host(master5, NR, NC, blob, offsets, "int", True, what)
        assert st[v] == -1 and (np.delete(st, v) == 0).all(), (what, st)
        _same_as_host(master5, NR, NC, blob, offsets, "int", False, what)
    # the framing rules one by one, the checksum made good again so that with verification on the framing is what decides:
    # (record, status of the victim with verification off; None: whatever the host says)
    cases = {
        "type byte 3": (_refresh_crc(r[:4] + b"\x03" + r[5:]), -1),
        "size + 4": (_put32(r, 0, size + 4), -2),
        "size 16": (_put32(r, 0, 16), -2),
        "n = size - 15": (_refresh_crc(_put32(r, 12, size - 15)), -2),
        "codec index = n_codecs": (_refresh_crc(r[:16] + b"\x05" + r[17:]), -1),
        "codec index of the NONE entry": (_refresh_crc(r[:16] + b"\x02" + r[17:]), -1),
        "n = 0": (_refresh_crc(_put32(r, 12, 0)), -1),
    }
    for what, (rec, want) in cases.items():
        blob, offsets = _concat(batch(rec))
        for verify in (False, True):
            _, _, st = _same_as_host(master5, NR, NC, blob, offsets, "int", verify, what)
            assert st[v] == want and (np.delete(st, v) == 0).all(), (what, verify, st)
    # a size field greater than the record's span (the next record starts where this one's size says it should not)
    rec = _put32(r, 0, size + 8)
    blob, offsets = _concat(batch(rec))
    _, _, st = _same_as_host(master5, NR, NC, blob, offsets, "int", False, "size > span")
    assert st[v] == -2 and (np.delete(st, v) == 0).all()
    # a span of 12 bytes
    blob, offsets = _concat(batch(r[:12]))
    for verify in (False, True):
        _, _, st = _same_as_host(master5, NR, NC, blob, offsets, "int", verify, "span 12")
        assert st[v] == -2 and (np.delete(st, v) == 0).all()
    # a file without codecs: every packing is GF_ERR_FORMAT, the standard form still reads
    bare = gridfour_amd.CodecMasterHip(codec_list=[], context=ctx)
    blob, offsets = _concat(good)
    _, _, st = _same_as_host(bare, NR, NC, blob, offsets, "int", True, "n_codecs = 0")
    assert [s == 0 for s in st] == [len(elements[i]) == std for i in range(12)] and set(st) <= {0, -1} and (st == -1).any()


def test_bad_offsets_are_per_record_bounds_errors(master5, mixed_int):
    """the documented difference from the host call (which refuses such an array as a whole)"""
    records, elements, tiles = mixed_int
    good = records[:6]
    blob, offsets = _concat(good)
    a = offsets.copy()
    a[1], a[2] = offsets[2], offsets[1]            # record 1 runs backwards; record 0 spans two records, record 2 starts at record 1's bytes
    idx, vals, st = master5.record_blob_dev(NR, NC, blob, a, verify_checksums=True)
    assert list(st) == [0, -2, 0, 0, 0, 0] and idx[1] == -1
    assert np.array_equal(vals[[0, 2, 3, 4, 5]], tiles[[0, 1, 3, 4, 5]])
    b = offsets.copy()
    b[-1] += 8                                     # the last record ends behind blob_bytes
    idx, vals, st = master5.record_blob_dev(NR, NC, blob, b, verify_checksums=True)
    assert list(st) == [0, 0, 0, 0, 0, -2] and idx[5] == -1 and np.array_equal(vals[:5], tiles[:5])


# ---------------------------------------------------------------- 4. damaged packings

def _damaged_records(kind, slot):
    import oracle
    r, c = 24, 36
    values = make_tile("smooth", r, c, seed=31).astype(np.int32)
    enc = {D.HUFFMAN: oracle.codec_huffman_encode, D.CANON: oracle.codec_canon_encode, D.DEFLATE: oracle.codec_deflate_encode}[kind]
    pk = enc(slot, r, c, values)
    pk = pk[0] if isinstance(pk, tuple) else pk
    cases = D.damage_set(pk, kind, r, c, seed=17)
    kept = [(label, p) for label, p in cases if D.deviation(p, kind, r * c) is None and len(p) != r * c * 4]
    return r, c, values, pk, cases, kept


@pytest.mark.parametrize("kind,slot", [(D.HUFFMAN, 0), (D.DEFLATE, 1), (D.CANON, 3)])
def test_damaged_packings_in_records(master5, kind, slot):
    r, c, values, pk, cases, kept = _damaged_records(kind, slot)
    assert len(cases) >= 100 and 4 * (len(cases) - len(kept)) <= len(cases), (len(cases), len(kept))
    records = [_frame(0, pk, crc=False)] + [_frame(1 + i, p, crc=False) for i, (_, p) in enumerate(kept)]
    blob, offsets = _concat(records)
    _, vals, st = _same_as_host(master5, r, c, blob, offsets, "int", False, kind)
    assert st[0] == 0 and np.array_equal(vals[0], values) and (st != 0).any()


def test_damaged_lsop_packings_in_records(ctx, master5):
    """LSOP12 containers (tests/damage.py has no generator for them): bit flips at a stride over the whole container, every
    bit of the header's first bytes, truncations"""
    import gridfour_amd
    r, c = 24, 36
    values = make_tile("smooth", r, c, seed=33).astype(np.int32)
    pk = gridfour_amd.LsCodecHip(context=ctx).encode_batch(4, r, c, values[None])[0][0]
    assert pk is not None and pk[0] == 4
    nb = len(pk) * 8
    flips = list(range(8, 8 * 8)) + list(range(64, nb, max(1, nb // 400) | 1))
    cases = [_flip(pk, i >> 3, i & 7) for i in flips] + [pk[:k] for k in (1, 2, 3, 54, 55, 58, 59, 60, len(pk) // 2, len(pk) - 1)]
    records = [_frame(0, pk, crc=False)] + [_frame(1 + i, p, crc=False) for i, p in enumerate(cases)]
    blob, offsets = _concat(records)
    _, vals, st = _same_as_host(master5, r, c, blob, offsets, "int", False, "lsop")
    assert st[0] == 0 and np.array_equal(vals[0], values) and (st != 0).any()


# ---------------------------------------------------------------- 5. alignment and garbage

@pytest.mark.parametrize("element", ["int", "short"])
def test_any_alignment_and_garbage_between_records(master5, mixed_int, mixed_short, element):
    records, elements, tiles = mixed_int if element == "int" else mixed_short
    good = records[:12]
    blob0, offsets0 = _concat(good)
    ref = {v: master5.record_blob_dev(NR, NC, blob0, offsets0, element=element, verify_checksums=v) for v in (True, False)}
    assert (ref[True][2] == 0).all()
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        parts, offsets, pos = [], [], 0
        for i, rec in enumerate(good):
            gap = int(rng.integers(1, 40))
            gap += (i % 8 - (pos + gap)) % 8            # record i starts at a byte offset = i mod 8
            parts.append(bytes(rng.integers(1, 256, gap, dtype=np.uint8)))
            pos += gap
            assert pos % 8 == i % 8
            offsets.append(pos)                         # its span runs through the filler to the next record
            parts.append(rec)
            pos += len(rec)
        parts.append(bytes(rng.integers(1, 256, 37, dtype=np.uint8)))
        offsets.append(pos + 37)
        blob = np.frombuffer(b"".join(parts), np.uint8)
        for verify in (True, False):
            got = _same_as_host(master5, NR, NC, blob, np.array(offsets, np.uint64), element, verify, "shifted")
            dev = master5.record_blob_dev(NR, NC, blob, np.array(offsets, np.uint64), element=element, verify_checksums=verify)
            for a, b, want in zip(got, dev, ref[verify]):
                assert np.array_equal(a, want) and np.array_equal(b, want)


# ---------------------------------------------------------------- 6. CRC run edges

@pytest.mark.parametrize("nr,nc,element", [(1, 1, "int"), (5, 5, "short"), (1, 63, "int"), (1, 64, "int"), (1, 65, "int"), (120, 150, "int")])
def test_crc_run_edges(ctx, nr, nc, element):
    import gridfour_amd
    master = gridfour_amd.CodecMasterHip(context=ctx)
    cells = nr * nc
    rng = np.random.default_rng(cells)
    if element == "short":
        v = rng.integers(-32767, 32768, cells).astype(np.int16)
        el = v.astype("<i2").tobytes() + b"\0" * (-2 * cells % 4)            # standard size: rounded up to a multiple of 4
    else:
        v = rng.integers(-2**31 + 1, 2**31, cells).astype(np.int32)
        el = v.astype("<i4").tobytes()
    rec = _frame(42, el)
    if (nr, nc) == (1, 1):
        assert len(rec) == 24
    if (nr, nc) == (5, 5):
        assert len(el) == 52
    stored = struct.unpack_from("<I", rec, len(rec) - 4)[0]
    assert stored == _crc32c(rec[:-4])                                        # gf_crc32c and the pure-Python twin agree
    bad = [_flip(rec, 16 + len(el) - 1, 7), _flip(rec, 0 + 9, 0), _flip(rec, len(rec) - 1, 3)]
    blob, offsets = _concat([rec] + bad + [rec])
    idx, vals, st = _same_as_host(master, nr, nc, blob, offsets, element, True, "crc")
    assert list(st) == [0, -1, -1, -1, 0]
    assert np.array_equal(vals[0], v) and np.array_equal(vals[4], v) and idx[0] == 42


# ---------------------------------------------------------------- 7. partition edges

def _small_tiles(n, r, c):
    kinds = ["smooth", "steps", "noise8", "ramp"]
    return np.stack([make_tile(kinds[i % 4], r, c, seed=100 + i) for i in range(n)]).astype(np.int32)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_partition_one_codec_only(ctx, n):
    """every record names the same codec: the partition is the identity and its decoder writes straight to the caller's arrays"""
    import gridfour_amd
    r, c = 16, 20
    master = gridfour_amd.CodecMasterHip(codec_list=(NONE, NONE, NONE, CANON), context=ctx)
    tiles = _small_tiles(n, r, c) if n else np.zeros((0, r * c), np.int32)
    records, used = master.tile_records(r, c, list(range(n)), tiles) if n else ([], np.zeros(0, np.uint8))
    assert (used == 3).all()
    blob, offsets = _concat(records)
    for verify in (True, False):
        idx, vals, st = _same_as_host(master, r, c, blob, offsets, "int", verify)
        assert (st == 0).all() and list(idx) == list(range(n)) and np.array_equal(vals, tiles)


def _alternating(ctx, n, r, c, slots):
    """n records whose codec changes from record to record: slots cycles over codec indices of LIST5 and None (standard form)"""
    import gridfour_amd
    tiles = _small_tiles(n, r, c)
    enc = {0: gridfour_amd.CodecHuffmanHip(context=ctx), 1: gridfour_amd.CodecDeflateHip(context=ctx),
           3: gridfour_amd.CodecCanonHuffmanHip(context=ctx), 4: gridfour_amd.LsCodecHip(context=ctx)}
    records = [None] * n
    for k, slot in enumerate(slots):
        members = list(range(k, n, len(slots)))
        if not members:
            continue
        packs = enc[slot].encode_batch(slot, r, c, tiles[members])[0] if slot is not None else [None] * len(members)
        for i, pk in zip(members, packs):
            records[i] = _frame(i, pk if pk is not None and len(pk) < r * c * 4 else tiles[i].astype("<i4").tobytes())
    return records, tiles


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_partition_alternating_codecs(ctx, master5, n):
    r, c = 16, 20
    records, tiles = _alternating(ctx, n, r, c, (0, 1, 3, 4, None))
    blob, offsets = _concat(records)
    idx, vals, st = _same_as_host(master5, r, c, blob, offsets, "int", True)
    assert (st == 0).all() and list(idx) == list(range(n)) and np.array_equal(vals, tiles)


def test_partition_codec_without_member_and_all_failed(ctx, master5):
    r, c = 16, 20
    records, tiles = _alternating(ctx, 65, r, c, (0, 3))            # the list's Deflate and LSOP12 entries have no member
    blob, offsets = _concat(records)
    idx, vals, st = _same_as_host(master5, r, c, blob, offsets, "int", True)
    assert (st == 0).all() and np.array_equal(vals, tiles)
    # every record fails the framing: no decoder runs, every status is set, no value is written
    broken = [rec[:4] + b"\x03" + rec[5:] for rec in records]
    blob, offsets = _concat(broken)
    idx, vals, st = _same_as_host(master5, r, c, blob, offsets, "int", False)
    assert (st == -1).all() and (idx == -1).all() and (vals == 0).all()


# ---------------------------------------------------------------- 8. context reuse

def test_context_reuse_and_buffer_growth(mixed_int):
    """the context's temporaries grow between batches; results do not change and the one-tile graphs survive the growth"""
    import gridfour_amd
    ctx = gridfour_amd.GvrsHipContext()
    master = gridfour_amd.CodecMasterHip(codec_list=LIST5, context=ctx)
    huff = gridfour_amd.CodecHuffmanHip(context=ctx)
    one = make_tile("smooth", NR, NC, seed=77).astype(np.int32)
    pk = huff.encode(0, NR, NC, one)
    assert np.array_equal(huff.decode(NR, NC, pk), one)
    records, elements, tiles = mixed_int
    blob, offsets = _concat(records)
    first = master.record_blob_dev(NR, NC, blob, offsets, verify_checksums=True)
    assert (first[2] == 0).all() and np.array_equal(first[1], tiles)
    again = master.record_blob_dev(NR, NC, blob, offsets, verify_checksums=True)
    # the three device entry points carve the same scratch buffers: several elements (one record holding the same element three
    # times), then packings without framing, between the one-element calls
    triple = [_frame_elems(7 * i, [el, el, el]) for i, el in enumerate(elements)]
    t_blob, t_offsets = _concat(triple)
    _, t_vals, t_st = master.record_blob_elems_dev(NR, NC, t_blob, t_offsets, ["int", "int", "int"], verify_checksums=True)
    assert (t_st == 0).all() and all(np.array_equal(v, tiles) for v in t_vals)
    packs = [el for el in elements if len(el) != NR * NC * 4]
    p_vals, p_st = master.decode_batch_dev(NR, NC, packs)
    assert (p_st == 0).all() and np.array_equal(p_vals, tiles[[len(el) != NR * NC * 4 for el in elements]])
    big_records, big_tiles = _alternating(ctx, 257, 64, 64, (0, 3, None, 4, 1))
    big_blob, big_offsets = _concat(big_records)
    idx, vals, st = master.record_blob_dev(64, 64, big_blob, big_offsets, verify_checksums=True)
    assert (st == 0).all() and np.array_equal(vals, big_tiles)
    _, t_vals, t_st = master.record_blob_elems_dev(NR, NC, t_blob, t_offsets, ["int", "int", "int"], verify_checksums=True)
    assert (t_st == 0).all() and all(np.array_equal(v, tiles) for v in t_vals)
    third = master.record_blob_dev(NR, NC, blob, offsets, verify_checksums=True)
    for a, b, c in zip(first, again, third):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert np.array_equal(huff.decode(NR, NC, pk), one)
    ctx.close()


# ---------------------------------------------------------------- 9. the scatter route at small shapes

SMALL = [(1, 1), (5, 5), (7, 9), (40, 60)]


@pytest.mark.parametrize("element", ["int", "short"])
@pytest.mark.parametrize("nr,nc", SMALL)
def test_scatter_route_at_small_shapes(ctx, master5, nr, nc, element):
    """a mixed batch (temporary + scatter) through the one-element entry points where cells is no multiple of 8 and a tile's bytes
    no multiple of 16: the scalar narrowing loop and the 8-, 4- and 1-byte copies of the scatter kernel.  Twenty records at byte
    offsets of every residue mod 8: four tiles offered to each integer codec of LIST5 (one that declines the shape or does not
    shorten the tile leaves it in standard form), three in standard form, one more whose stored checksum has a flipped bit."""
    import gridfour_amd
    cells, short = nr * nc, element == "short"
    std = (2 * cells + 3) & ~3 if short else 4 * cells
    kinds = ["smooth", "uniform", "noise8", "steps", "ramp"]
    tiles = np.stack([make_tile(kinds[i % 5], nr, nc, seed=500 + i) for i in range(19)]).astype(np.int32)
    if short:
        tiles = np.clip(tiles, -32767, 32767)
    tiles[2, 0] = tiles[11, cells // 2] = tiles[17, cells - 1] = NULL
    enc = {0: gridfour_amd.CodecHuffmanHip(context=ctx), 1: gridfour_amd.CodecDeflateHip(context=ctx),
           3: gridfour_amd.CodecCanonHuffmanHip(context=ctx), 4: gridfour_amd.LsCodecHip(context=ctx)}
    packings = sum((codec.encode_batch(slot, nr, nc, tiles[4 * k:4 * k + 4])[0] for k, (slot, codec) in enumerate(enc.items())), []) + [None] * 3
    elements = []
    for tile, pk in zip(tiles, packings):
        if pk is not None and len(pk) < std:
            elements.append(pk)
        elif short:
            elements.append(np.where(tile == NULL, -32768, tile).astype("<i2").tobytes() + b"\0" * (std - 2 * cells))
        else:
            elements.append(tile.astype("<i4").tobytes())
    n_packed = sum(len(el) != std for el in elements)
    assert n_packed <= 16 and (n_packed >= 1 or (nr, nc) == (1, 1)), n_packed      # (and at least three in standard form)
    records = [_frame(300 + 5 * i, el) for i, el in enumerate(elements)]
    records.append(_flip(records[-1], len(records[-1]) - 2, 4))
    blob, offsets = _shifted(records, seed=cells)
    assert {int(o) % 8 for o in offsets[:-1]} == set(range(8))
    want = np.where(tiles == NULL, -32768, tiles).astype(np.int16) if short else tiles
    for verify in (True, False):
        idx, vals, st = _same_as_host(master5, nr, nc, blob, offsets, element, verify, (nr, nc))
        assert list(st) == [0] * 19 + [-1 if verify else 0], st
        assert list(idx) == [300 + 5 * i for i in range(19)] + [300 + 5 * 18]
        assert np.array_equal(vals[:19], want) and (not verify or (vals[19] == 0).all())
    packs = [el for el in elements if len(el) != std]
    if packs:
        hv, hs = master5.decode_batch(nr, nc, packs)
        dv, ds = master5.decode_batch_dev(nr, nc, packs)
        assert (hs == 0).all() and np.array_equal(ds, hs) and np.array_equal(dv, hv)
        assert np.array_equal(dv, tiles[[len(el) != std for el in elements]])
