"""Tile records of several elements WRITTEN on the GPU (gf_tile_record_encode_batch_elems_dev and its host form): byte for byte
against the oracle's packings framed in Python (tests/records_enc_inputs.py -- expected bytes never come from the code under test),
the reference's own sample files re-encoded, the one-element call gf_tile_record_encode_batch, a round trip through the read side
in device memory, the capacity rule, records without checksums, the verdicts, and context reuse."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import records_enc_inputs as R
from gvrs_walk import walk_records
from test_gpu_records_dev import LIST5, NC, NR, _frame_elems, _source_tiles
from test_gpu_records_elems import ICF1, _bits, _icf_expect
from tilegen import make_tile

pytestmark = pytest.mark.gpu
NULL = -2**31
HC = (R.HUFFMAN, R.CANON)
STANDARD = (R.HUFFMAN, R.DEFLATE, R.NONE, R.CANON)


def _p(a):
    return C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def ctx():
    import gridfour_amd
    return gridfour_amd.GvrsHipContext()


def _master(ctx, codecs):
    import gridfour_amd
    return gridfour_amd.CodecMasterHip(codec_list=list(codecs), context=ctx)


def _dev(master, batch, checksums=True, blob_cap=None):
    """(blob with its 0xA5 filler, offsets, codec_used, status) of the device form"""
    return master.tile_records_elems_dev(batch.nr, batch.nc, batch.indices, batch.values, batch.elems, checksums=checksums,
                                         blob_cap=blob_cap, raw=True)


def _offsets_of(records):
    off = np.zeros(len(records) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in records])
    return off


def _assert_exact(got, records, used, what):
    blob, offsets, g_used, status = got
    want_off = _offsets_of(records)
    assert (status == 0).all(), (what, status[status != 0][:8])
    assert np.array_equal(offsets, want_off), (what, offsets[:4], want_off[:4])
    assert np.array_equal(g_used, used), (what, np.argwhere(g_used != used)[:4])
    total = int(want_off[-1])
    want = np.frombuffer(b"".join(records), np.uint8)
    if not np.array_equal(blob[:total], want):
        at = int(np.argmax(blob[:total] != want))
        t = int(np.searchsorted(want_off, at, side="right")) - 1
        raise AssertionError((what, "first differing byte", at, "record", t, "at", at - int(want_off[t]), "of", len(records[t])))
    assert (blob[total:] == 0xA5).all(), (what, "bytes behind the last record were written")


# ---------------------------------------------------------------- 1. the oracle's packings framed in Python, byte for byte

CASES1 = [(codecs, name, shape) for codecs in R.LISTS for name in R.ELEMENT_SETS for shape in R.SHAPES
          if not (R.NONE in codecs and name == "three")]


@pytest.mark.parametrize("codecs,name,shape", CASES1, ids=["%s-%s-%dx%d" % ("".join(map(str, c)), n, s[0], s[1]) for c, n, s in CASES1])
def test_oracle_framing_byte_for_byte(ctx, codecs, name, shape):
    master = _master(ctx, codecs)
    pool = R.pool(name, *shape)
    for set_name, sh, nt in R.gpu_batches():
        if set_name != name or sh != shape:
            continue
        if nt == 1025 and codecs != (R.CANON, R.HUFFMAN):           # (the scan's second block: once per element set)
            continue
        batch = pool.head(nt)
        records, used = batch.expected(codecs)
        _assert_exact(_dev(master, batch), records, used, (codecs, name, shape, nt))


def test_host_form_equals_the_oracle_framing(ctx):
    """a list the device form accepts, through the host form: staged into the context's buffers and sent through the same kernels"""
    master = _master(ctx, HC)
    for name, shape in (("three", (7, 9)), ("sixteen", (16, 20)), ("short", (40, 60))):
        batch = R.pool(name, *shape).head(65)
        records, used = batch.expected(HC)
        got, g_used = master.tile_records_elems(batch.nr, batch.nc, batch.indices, batch.values, batch.elems)
        assert got == records and np.array_equal(g_used, used), (name, shape)


# ---------------------------------------------------------------- 2. the reference's own files

def _file_records(golden_dir, name):
    with open(os.path.join(golden_dir, "ref_samples", name), "rb") as f:
        data = f.read()
    spans = sorted((pos, size) for pos, size, rtype, _ in walk_records(data) if rtype == 2)
    return [data[p:p + s] for p, s in spans]


UNCOMPRESSED = [
    # file, tile size, elements as the file has them, checksums
    ("Sample00_ShortNoComp.gvrs", 5, ["short"], True),
    ("Sample01_IntNoComp.gvrs", 5, ["int"], True),
    ("Sample02_FltNoComp.gvrs", 5, ["float"], True),
    ("Sample03_ICFNoComp.gvrs", 5, [ICF1], True),
    ("Sample08_MixedTypes.gvrs", 5, ["short", "float"], False),        # (the file's CRC words are zero)
    ("Sample09_ShortNoComp.gvrs", 6, ["short"], True),
    ("Sample10_IntNoComp.gvrs", 6, ["int"], True),
    ("Sample11_FltNoComp.gvrs", 6, ["float"], True),
    ("Sample12_ICFNoComp.gvrs", 6, [ICF1], True),
    ("Sample13_ModelCoord.gvrs", 11, ["float"], True),
]
COMPRESSED = [
    ("Sample04_ShortComp.gvrs", 50, ["short"], True),
    ("Sample05_IntComp.gvrs", 50, ["int"], True),
    ("Sample06_FltComp.gvrs", 50, ["float"], True),
    ("Sample07_ICFComp.gvrs", 50, [ICF1], True),
]


def _decode_file(ctx, codecs, records, tile, elems, verify):
    """the file's records read back on the device; an int-coded-float element as the int codes it stores"""
    as_int = ["int" if not isinstance(el, str) else el for el in elems]
    blob = np.frombuffer(b"".join(records), np.uint8)
    idx, vals, st = _master(ctx, codecs).record_blob_elems_dev(tile, tile, blob, _offsets_of(records), as_int, verify_checksums=verify)
    assert (st == 0).all()
    return idx, vals, as_int


@pytest.mark.parametrize("name,tile,elems,crc", UNCOMPRESSED, ids=[c[0][:8] for c in UNCOMPRESSED])
def test_reference_files_without_compression(golden_dir, ctx, name, tile, elems, crc):
    """decoded on the device, re-encoded by the DEVICE form with an empty codec list: the file's bytes"""
    records = _file_records(golden_dir, name)
    assert len(records) == (1 if name.startswith("Sample13") else 4)
    idx, vals, as_int = _decode_file(ctx, [], records, tile, elems, crc)
    got, used, st = _master(ctx, []).tile_records_elems_dev(tile, tile, idx, vals, as_int, checksums=crc)
    assert (st == 0).all() and (used == 255).all()
    assert got == records
    if name.startswith("Sample08"):
        assert all(struct.unpack_from("<i", r, 12)[0] == 52 and struct.unpack_from("<I", r, len(r) - 4)[0] == 0 for r in got)


@pytest.mark.parametrize("name,tile,elems,crc", COMPRESSED, ids=[c[0][:8] for c in COMPRESSED])
def test_reference_files_with_compression(golden_dir, ctx, name, tile, elems, crc):
    """decoded on the device, re-encoded by the HOST form under the standard list (CodecDeflate / CodecFloat need the host's zlib)"""
    records = _file_records(golden_dir, name)
    assert len(records) == 4
    idx, vals, as_int = _decode_file(ctx, STANDARD, records, tile, elems, crc)
    got, used = _master(ctx, STANDARD).tile_records_elems(tile, tile, idx, vals, as_int, checksums=crc)
    assert (used != 255).all()
    assert got == records


# ---------------------------------------------------------------- 3. the one-element call

@pytest.mark.parametrize("element", ["int", "short"])
def test_equals_the_one_element_call(ctx, element):
    tiles, _ = _source_tiles(element)
    idx = [1000 + 7 * i for i in range(len(tiles))]
    vals = np.where(tiles == NULL, -32768, tiles).astype(np.int16) if element == "short" else tiles
    for codecs in (LIST5, HC):
        master = _master(ctx, codecs)
        old, old_used = master.tile_records(NR, NC, idx, vals, element=element, fill_value=-32768)
        new, new_used = master.tile_records_elems(NR, NC, idx, [vals], [element])
        assert new == old and np.array_equal(new_used[0], old_used), (element, codecs)
        assert len({u for u in old_used}) >= 3                                            # several codecs and the standard form
    dev, dev_used, st = master.tile_records_elems_dev(NR, NC, idx, [vals], [element])
    assert (st == 0).all() and dev == old and np.array_equal(dev_used[0], old_used)


# ---------------------------------------------------------------- 4. round trip in device memory

@pytest.mark.parametrize("shape", R.SHAPES, ids=["%dx%d" % s for s in R.SHAPES])
def test_round_trip_in_device_memory(ctx, shape):
    """the device form's blob goes straight into gf_tile_record_decode_batch_elems_dev, checksums verified"""
    from gridfour_amd import DeviceBuffer
    from gridfour_amd._lib import check, lib
    batch = R.pool("three", *shape).head(65)
    master = _master(ctx, HC)
    nr, nc = shape
    nt, ne, cells = batch.nt, 3, nr * nc
    specs, vals = master._elem_values(nr, nc, batch.values, batch.elems, None)
    cap = nt * int(lib().gf_tile_record_max_bytes_elems(_p(specs), ne, nr, nc))
    d_val = [DeviceBuffer(ctx, v.nbytes + 16).upload(v) for v in vals]
    d_idx = DeviceBuffer(ctx, nt * 4 + 16).upload(batch.indices)
    d_blob = DeviceBuffer(ctx, cap + 64).fill(0xA5)
    d_off = DeviceBuffer(ctx, (nt + 1) * 8 + 16)
    d_st = DeviceBuffer(ctx, nt * 4 + 16)
    out_dt = [np.int16, np.float32, np.float32]
    d_out = [DeviceBuffer(ctx, nt * cells * np.dtype(dt).itemsize + 16).fill(0) for dt in out_dt]
    d_idx2 = DeviceBuffer(ctx, nt * 4 + 16).fill(0xff)
    d_st2 = DeviceBuffer(ctx, ne * nt * 4 + 16).fill(0x7f)
    ptrs = (C.c_void_p * ne)(*[b.ptr.value for b in d_val])
    outs = (C.c_void_p * ne)(*[b.ptr.value for b in d_out])
    codecs = np.array(HC, np.int32)
    try:
        check(lib().gf_tile_record_encode_batch_elems_dev(ctx.handle, None, _p(codecs), 2, _p(specs), ne, nr, nc, nt, d_idx.ptr, ptrs, 1,
                                                          d_blob.ptr, cap, d_off.ptr, None, d_st.ptr), "encode")
        ctx.synchronize()
        total = int(d_off.download(np.uint64, nt + 1)[nt])                                # (blob_bytes is a host argument)
        assert 0 < total <= cap and (d_st.download(np.int32, nt) == 0).all()
        check(lib().gf_tile_record_decode_batch_elems_dev(ctx.handle, None, _p(codecs), 2, _p(specs), ne, nr, nc, nt, d_blob.ptr, total,
                                                          d_off.ptr, 1, d_idx2.ptr, outs, d_st2.ptr), "decode")
        ctx.synchronize()
        assert (d_st2.download(np.int32, ne * nt) == 0).all()
        assert np.array_equal(d_idx2.download(np.int32, nt), batch.indices)
        got = [b.download(dt, nt * cells).reshape(nt, cells) for b, dt in zip(d_out, out_dt)]
    finally:
        for b in [d_idx, d_blob, d_off, d_st, d_idx2, d_st2] + d_val + d_out:
            b.free()
    assert np.array_equal(got[0], batch.values[0])                                        # (fill = -32768 = what a null decodes to)
    assert np.array_equal(_bits(got[1]), _bits(_icf_expect(batch.values[1], R.ICF3)))
    f = _bits(batch.values[2])
    assert np.array_equal(_bits(got[2]), f)
    assert (f == 0x80000000).any() and (f == 0x7fc12345).any() and (f == 0xffa00001).any()  # -0.0 and NaN payloads among the cells


# ---------------------------------------------------------------- 5. capacity

def test_capacity(ctx):
    from gridfour_amd._lib import ERR_CAPACITY, lib
    batch = R.pool("three", 16, 20).head(65)
    master = _master(ctx, HC)
    records, used = batch.expected(HC)
    want_off = _offsets_of(records)
    mid = batch.nt // 2
    cap = int(want_off[mid]) + 3
    blob, offsets, g_used, status = _dev(master, batch, blob_cap=cap)
    assert np.array_equal(offsets, want_off) and int(offsets[batch.nt]) > cap             # complete, and it tells the caller
    assert (status == 0).all() and np.array_equal(g_used, used)
    fits = [t for t in range(batch.nt) if int(want_off[t + 1]) <= cap]
    assert fits == list(range(mid))
    assert bytes(blob[:int(want_off[mid])]) == b"".join(records[:mid])                    # every record that fits is exact
    assert (blob[int(want_off[mid]):] == 0xA5).all()                                       # nothing from the first skipped record on
    # the host form: GF_ERR_CAPACITY with offsets[n] filled in
    specs, vals = master._elem_values(batch.nr, batch.nc, batch.values, batch.elems, None)
    h_blob = np.full(cap + 64, 0xA5, np.uint8)
    h_off = np.zeros(batch.nt + 1, np.uint64)
    ptrs = (C.c_void_p * 3)(*[a.ctypes.data for a in vals])
    codecs = np.array(HC, np.int32)
    s = lib().gf_tile_record_encode_batch_elems(ctx.handle, _p(codecs), 2, _p(specs), 3, batch.nr, batch.nc, batch.nt, _p(batch.indices), ptrs,
                                                1, _p(h_blob), cap, _p(h_off), None)
    assert s == ERR_CAPACITY and np.array_equal(h_off, want_off) and (h_blob[cap:] == 0xA5).all()


# ---------------------------------------------------------------- 6. records without checksums

def test_without_checksums(ctx):
    batch = R.pool("three", 7, 9).head(64)
    master = _master(ctx, (R.CANON, R.HUFFMAN))
    with_crc, used = batch.expected((R.CANON, R.HUFFMAN))
    without, _ = batch.expected((R.CANON, R.HUFFMAN), crc=False)
    assert all(a[:-4] == b[:-4] and b[-4:] == b"\0\0\0\0" and a[-4:] != b[-4:] for a, b in zip(with_crc, without))
    _assert_exact(_dev(master, batch, checksums=False), without, used, "checksum_enabled = 0")


# ---------------------------------------------------------------- 7. verdicts

def _host_plan(batch, codecs, float_level=6):
    """the oracle's framing for lists the device form refuses: Deflate among the integer codecs, CodecFloat at the first NONE entry"""
    import oracle
    enc = {R.HUFFMAN: oracle.codec_huffman_encode, R.CANON: oracle.codec_canon_encode, R.DEFLATE: oracle.codec_deflate_encode}
    cells = batch.nr * batch.nc
    fslot = next((k for k, c in enumerate(codecs) if c == R.NONE), None)
    records, used = [], np.full((len(batch.elems), batch.nt), 255, np.uint8)
    for t in range(batch.nt):
        parts = []
        for e, el in enumerate(batch.elems):
            std = R.std_size(el, cells)
            best, best_k = None, 255
            if R.kind_of(el) == "float":
                if fslot is not None:
                    best, best_k = oracle.codec_float_encode(fslot, batch.nr, batch.nc, _bits(batch.values[e][t]), level=float_level), fslot
            else:
                v = R.codec_cells(el, batch.values[e][t])
                for k, c in enumerate(codecs):
                    if c in enc:
                        pk = enc[c](k, batch.nr, batch.nc, v)
                        pk = pk[0] if isinstance(pk, tuple) else pk
                        if pk is not None and (best is None or len(pk) < len(best)):
                            best, best_k = pk, k
            if best is not None and len(best) < std:
                parts.append(best)
                used[e, t] = best_k
            else:
                parts.append(R.standard_form(el, batch.values[e][t]))
        records.append(_frame_elems(int(batch.indices[t]), parts))
    return records, used


def test_lists_the_device_form_refuses_go_through_the_host_form(ctx):
    from gridfour_amd import GvrsHipError
    from gridfour_amd._lib import ERR_UNSUPPORTED
    batch = R.pool("three", 16, 20).head(24)
    ints = R.pool("int", 16, 20).head(24)
    for codecs, b in ((STANDARD, batch), ((R.HUFFMAN, R.DEFLATE), ints), ((R.LSOP, R.CANON), ints), ((R.CANON, R.NONE), batch)):
        master = _master(ctx, codecs)
        with pytest.raises(GvrsHipError) as err:
            _dev(master, b)
        assert err.value.status == ERR_UNSUPPORTED, codecs
        got, used = master.tile_records_elems(b.nr, b.nc, b.indices, b.values, b.elems)
        if R.LSOP not in codecs:
            # (CodecDeflate and CodecFloat are held to the oracle on this zlib by tests/test_gpu_deflate.py and tests/test_gpu_float.py)
            want, want_used = _host_plan(b, codecs)
            assert got == want and np.array_equal(used, want_used), codecs
        # ... and every one of them reads back
        as_int = ["int" if not isinstance(el, str) else el for el in b.elems]
        blob = np.frombuffer(b"".join(got), np.uint8)
        idx, vals, st = master.record_blob_elems_dev(b.nr, b.nc, blob, _offsets_of(got), as_int, verify_checksums=True)
        assert (st == 0).all() and np.array_equal(idx, b.indices)
        for e, el in enumerate(b.elems):
            assert np.array_equal(_bits(vals[e]), _bits(b.values[e])) if el == "float" else np.array_equal(vals[e], b.values[e]), (codecs, e)
    assert (used[:, :] != 255).any()


def test_an_encoder_that_fails_fails_its_record_alone(ctx):
    """16 x 1 tiles: PredictorModelLinear indexes values[1] (ArrayIndexOutOfBounds) unless the tile has nulls -- the encoders report
    GF_ERR_BOUNDS per tile at this shape, so such a record has length 0 and its neighbours are written"""
    nr, nc, nt = 16, 1, 12
    tiles = np.stack([make_tile("noise8", nr, nc, seed=i) for i in range(nt)]).astype(np.int32)
    good = [1, 4, 5, 9, 11]
    for t in good:
        tiles[t, (3 * t) % nr] = NULL
    tiles[9, :] = NULL                                                                  # every codec declines: the standard form
    batch = R.Batch.__new__(R.Batch)
    batch.elems, batch.nr, batch.nc, batch.nt, batch.values, batch._cand = ["int"], nr, nc, nt, [tiles], {}
    batch.indices = np.arange(nt, dtype=np.int32)
    master = _master(ctx, HC)
    blob, offsets, used, status = _dev(master, batch)
    assert [int(s) for s in status] == [0 if t in good else -2 for t in range(nt)]
    sub = R.Batch.__new__(R.Batch)                                                     # (the oracle throws on the others, as Java does)
    sub.elems, sub.nr, sub.nc, sub.nt, sub.values, sub._cand = ["int"], nr, nc, len(good), [tiles[good]], {}
    plan = dict(zip(good, sub.plan(HC)[0]))
    pos = 0
    for t in range(nt):
        if t not in good:
            assert offsets[t + 1] == offsets[t]
            continue
        want = _frame_elems(t, [plan[t][0]])
        assert int(offsets[t]) == pos and bytes(blob[pos:pos + len(want)]) == want and used[0, t] == plan[t][1]
        pos += len(want)
    assert int(offsets[nt]) == pos and (blob[pos:] == 0xA5).all() and used[0, 9] == 255
    # the host form returns the first negative per-tile status as its own
    from gridfour_amd import GvrsHipError
    with pytest.raises(GvrsHipError) as err:
        master.tile_records_elems(nr, nc, batch.indices, batch.values, batch.elems)
    assert err.value.status == -2


def test_an_unaligned_blob_is_refused(ctx):
    from gridfour_amd import DeviceBuffer
    from gridfour_amd._lib import ERR_ARG, lib
    batch = R.pool("int", 7, 9).head(4)
    master = _master(ctx, HC)
    specs, vals = master._elem_values(7, 9, batch.values, batch.elems, None)
    d_val = DeviceBuffer(ctx, vals[0].nbytes + 16).upload(vals[0])
    d_idx = DeviceBuffer(ctx, 64).upload(batch.indices)
    d_blob = DeviceBuffer(ctx, 4096).fill(0xA5)
    d_off = DeviceBuffer(ctx, 64).fill(0xA5)
    d_st = DeviceBuffer(ctx, 64).fill(0xA5)
    ptrs = (C.c_void_p * 1)(d_val.ptr.value)
    codecs = np.array(HC, np.int32)
    try:
        for shift in (1, 4):
            s = lib().gf_tile_record_encode_batch_elems_dev(ctx.handle, None, _p(codecs), 2, _p(specs), 1, 7, 9, 4, d_idx.ptr, ptrs, 1,
                                                            C.c_void_p(d_blob.ptr.value + shift), 2048, d_off.ptr, None, d_st.ptr)
            assert s == ERR_ARG
        ctx.synchronize()
        assert (d_blob.download(np.uint8, 4096) == 0xA5).all() and (d_off.download(np.uint8, 64) == 0xA5).all()
    finally:
        for b in (d_val, d_idx, d_blob, d_off, d_st):
            b.free()


# ---------------------------------------------------------------- 8. context reuse

def test_context_reuse_and_buffer_growth():
    """the context's temporaries grow between batches; the bytes do not change and the one-tile graphs survive the growth"""
    import gridfour_amd
    ctx = gridfour_amd.GvrsHipContext()
    master = _master(ctx, HC)
    huff = gridfour_amd.CodecHuffmanHip(context=ctx)
    one = make_tile("smooth", NR, NC, seed=77).astype(np.int32)
    pk = huff.encode(0, NR, NC, one)
    assert np.array_equal(huff.decode(NR, NC, pk), one)
    small = R.pool("three", 7, 9).head(8)
    big = R.pool("sixteen", 40, 60).head(65)
    want_small, used_small = small.expected(HC)
    first = _dev(master, small)
    _assert_exact(first, want_small, used_small, "small")
    want_big, used_big = big.expected(HC)
    _assert_exact(_dev(master, big), want_big, used_big, "big")
    host, host_used = master.tile_records_elems(small.nr, small.nc, small.indices, small.values, small.elems)
    assert host == want_small
    again = _dev(master, small)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    assert huff.encode(0, NR, NC, one) == pk and np.array_equal(huff.decode(NR, NC, pk), one)
    ctx.close()
