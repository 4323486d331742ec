"""Batches that cross the seam of the bounded inflate scratch, one test per decode driver.

deflateDecodeDev (gvrs_api_deflate.hip), floatDecodeDev (gvrs_api_float.hip) and lsopUnpackM32Deflate (gvrs_api_lsop.hip) send a
batch through a fixed scratch in chunks of tiles; from the second chunk on every pointer and index carries the chunk's first
tile t0 (d_values + t0 * cells, d_status + t0, offsets[t0 + i] against descriptor i, d_residuals + t0 * stride, d_coefs + t0 * 16,
the slot form's d_blob + t0 * slot_stride), and the float driver clears the plane scratch per chunk so that a short stream reads
zeros behind its end.  The byte volume that reaches the second chunk is fixed by the scratch constants; the host-side cost is
not: a dozen distinct packings are uploaded once and the batch is described through d_offsets / d_lengths that point into that
small blob, the packing of tile t drawn from a seeded generator such that no tile of the second chunk holds the packing of the
tile one chunk before it.

The verdict rule is the decode contract of DESIGN.md 2, for EVERY tile: where the oracle decodes a packing the device reports 0
and the same cells; where it declines, 1; where it throws, GF_ERR_FORMAT or GF_ERR_BOUNDS.  The oracle decodes each distinct
packing once."""
import zlib

import numpy as np
import pytest

import float_ref
import oracle
from tilegen import make_tile

pytestmark = pytest.mark.gpu

GUARD = 4096                                     # bytes behind the last tile's cells and statuses
SENTINEL = 0x5A
INFLATE_SCRATCH_BYTES = 1 << 30                  # gvrs_api_internal.h: CodecDeflate, CodecFloat
LSOP_INFLATE_SCRATCH_BYTES = 384 << 20           # gvrs_api_lsop.hip


def _round16(x):
    return (x + 15) // 16 * 16


class _Pack:
    """a distinct packing and the oracle's verdict on it: cells (decodes), "null" (declines) or None (throws)"""

    def __init__(self, label, data, verdict):
        self.label, self.data, self.verdict = label, bytes(data), verdict
        self.ok = isinstance(verdict, np.ndarray)


def _verdict(decode_rc, cells, dtype, data):
    out = np.zeros(cells, dtype)
    rc = decode_rc(oracle._u8(data), out)
    return out if rc == oracle.OK else "null" if rc == oracle.DECLINED else None


def _sequence(seed, nt, chunk, packs, placed):
    """Which packing every tile holds: seeded draws over all of them, the hand-placed tiles on top, and then no tile of a later
    chunk equal to the tile a whole number of chunks before it -- a result that lands t0 tiles off, or a descriptor read t0
    tiles off, cannot go unnoticed."""
    rng = np.random.default_rng(seed)
    seq = rng.integers(0, len(packs), nt)
    for t, k in placed.items():
        seq[t] = k
    for t in range(chunk, nt):
        for back in range(t - chunk, -1, -chunk):
            if seq[back] == seq[t]:
                assert back not in placed or t not in placed, (back, t)
                fix = back if back not in placed else t
                seq[fix] = (seq[fix] + 1 + int(rng.integers(0, len(packs) - 1))) % len(packs)
    for shift in range(chunk, nt, chunk):
        assert (seq[shift:] != seq[:nt - shift]).all()
    for t, k in placed.items():
        assert seq[t] == k
    return seq


def _small_blob(packs):
    """the distinct packings back to back (no alignment: the ABI asks for none): blob, start of each, length of each"""
    lens = np.array([len(p.data) for p in packs], np.uint32)
    starts = np.zeros(len(packs), np.uint64)
    starts[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    blob = np.frombuffer(b"".join(p.data for p in packs) + bytes(64), np.uint8)
    return blob, starts, lens


def _check_tiles(packs, seq, vals, st, where):
    """the verdict rule, every tile"""
    ok = np.array([p.ok for p in packs])
    null = np.array([p.verdict == "null" if not p.ok else False for p in packs])
    k = np.asarray(seq)
    bad = np.nonzero(np.where(ok[k], st != 0, np.where(null[k], st != 1, (st != -1) & (st != -2))))[0]
    assert bad.size == 0, (where, "status", bad.size, [(int(t), packs[seq[t]].label, int(st[t])) for t in bad[:10]])
    wrong = [t for t in range(len(seq)) if ok[seq[t]] and not np.array_equal(vals[t], packs[seq[t]].verdict)]
    assert not wrong, (where, "cells", len(wrong), [(t, packs[seq[t]].label) for t in wrong[:10]])


def _guards(d_val, val_bytes, d_st, nt, where):
    assert (d_val.download(np.uint8, GUARD, val_bytes) == SENTINEL).all(), (where, "cells written past the last tile")
    assert (d_st.download(np.uint8, GUARD, nt * 4) == SENTINEL).all(), (where, "status written past the last tile")


def _run_offsets(ctx, call, cells, dtype, packs, seq, where):
    """One call of a device entry point in the offsets form over the small blob; checks every tile and the guard regions."""
    from gridfour_amd import DeviceBuffer as B
    nt = len(seq)
    blob, starts, lens = _small_blob(packs)
    d_blob = B(ctx, blob.nbytes).upload(blob)
    d_off = B(ctx, nt * 8 + 16).upload(starts[seq])
    d_len = B(ctx, nt * 4 + 16).upload(lens[seq])
    d_val = B(ctx, nt * cells * 4 + GUARD).fill(SENTINEL)
    d_st = B(ctx, nt * 4 + GUARD).fill(SENTINEL)
    call(nt, d_blob.ptr, blob.nbytes, d_off.ptr, 0, d_len.ptr, d_val.ptr, d_st.ptr)
    ctx.synchronize()
    vals = d_val.download(dtype, nt * cells).reshape(nt, cells)
    st = d_st.download(np.int32, nt)
    _guards(d_val, nt * cells * 4, d_st, nt, where)
    for b in (d_blob, d_off, d_len, d_val, d_st):
        b.free()
    _check_tiles(packs, seq, vals, st, where)


def _index(packs, label):
    return [p.label for p in packs].index(label)


def _seam_placements(packs, nt, chunk, intact, damaged):
    """around the seam and at the end: an intact packing followed by a damaged one, a damaged one followed by an intact one"""
    i, d = [_index(packs, x) for x in intact], [_index(packs, x) for x in damaged]
    return {chunk - 2: d[0], chunk - 1: i[0], chunk: d[1 % len(d)], chunk + 1: i[1], chunk + 2: i[2], chunk + 3: d[2 % len(d)],
            nt - 3: d[0], nt - 2: i[3], nt - 1: d[1 % len(d)]}


# ---- CodecDeflate ------------------------------------------------------------------------------------------------------------

def test_deflate_batch_crosses_the_scratch_seam():
    """gf_deflate_decode_batch_i32_dev, 120 x 150: stride = roundUp(10 + 6 * cells, 16) = 108,016 bytes of scratch a tile,
    chunk = 2^30 / 108,016 = 9,940 tiles; 9,980 tiles."""
    import gridfour_amd
    from gridfour_amd import lib
    from gridfour_amd._lib import check
    nr, nc, nt = 120, 150, 9980
    cells = nr * nc
    stride = _round16(10 + 6 * cells)
    chunk = INFLATE_SCRATCH_BYTES // stride
    assert (stride, chunk) == (108016, 9940) and nt * stride > INFLATE_SCRATCH_BYTES and chunk + 8 < nt < 2 * chunk
    codec = gridfour_amd.CodecDeflateHip()
    ctx = codec.ctx
    tiles = np.concatenate([oracle.dem_tiles(oracle.DEM_SEED + 4, nr, nc, 8, 0, 5),
                            np.stack([make_tile(k, nr, nc) for k in ("smooth", "noise8", "steps")])])
    tiles[3, 100:200] = -(2 ** 31)                                   # nulls predictor
    encoded, _, est = codec.encode_batch(0, nr, nc, tiles)
    assert (est == 0).all()

    def rc(p, out):
        return oracle.lib().gvo_codec_deflate_decode(nr, nc, oracle._p(p, oracle.C.c_uint8), p.size, oracle._p(out, oracle.C.c_int32))
    packs = []
    for t, pk in enumerate(encoded):
        assert bytes(pk) == oracle.codec_deflate_encode(0, nr, nc, tiles[t])[0], t
        packs.append(_Pack("intact %d" % t, pk, _verdict(rc, cells, np.int32, pk)))
        assert np.array_equal(packs[-1].verdict, tiles[t])
    a, b = bytes(encoded[1]), bytes(encoded[6])
    flipped = bytearray(a)
    flipped[-1] ^= 0x10
    for label, data in (("adler", flipped), ("header cut", a[:7]), ("ends early", b[:len(b) // 2]), ("ends early 2", a[:len(a) * 2 // 3])):
        packs.append(_Pack(label, data, _verdict(rc, cells, np.int32, data)))
    assert packs[_index(packs, "adler")].verdict is None and packs[_index(packs, "header cut")].verdict is None
    early = packs[_index(packs, "ends early")]                       # Inflater gives what it has; the rest of new byte[nM32] is zero
    assert early.ok and not np.array_equal(early.verdict, tiles[6])
    placed = _seam_placements(packs, nt, chunk, ["intact 0", "intact 3", "intact 5", "intact 7"], ["adler", "ends early", "header cut"])
    seq = _sequence(20260, nt, chunk, packs, placed)

    def call(n, d_blob, blob_bytes, d_off, slot, d_len, d_val, d_st):
        check(lib().gf_deflate_decode_batch_i32_dev(ctx.handle, None, nr, nc, n, d_blob, blob_bytes, d_off, slot, d_len, d_val, d_st),
              "gf_deflate_decode_batch_i32_dev")
    _run_offsets(ctx, call, cells, np.int32, packs, seq, "deflate, %d tiles" % nt)
    # the grown scratch serves a later, small call
    small = [_index(packs, x) for x in ("ends early", "intact 2", "adler", "ends early 2", "intact 6")]
    _run_offsets(ctx, call, cells, np.int32, packs, np.array(small), "deflate, 5 tiles behind")


# ---- CodecFloat --------------------------------------------------------------------------------------------------------------

def test_float_batch_crosses_the_scratch_seam():
    """gf_float_decode_batch_f32_dev, 120 x 152: stride = roundUp(ceil(cells / 8) + 4 * cells, 16) = 75,248 bytes of plane scratch
    a tile, chunk = 2^30 / 75,248 = 14,269 tiles; 14,300 tiles.  The driver clears the scratch per chunk: a packing whose sign plane
    inflates short sits at tile chunk + i where tile i was intact with sign bits set all over -- its tail must read as the zeros of
    Java's fresh array, not as what tile i left in slot i."""
    import gridfour_amd
    from gridfour_amd import lib
    from gridfour_amd._lib import check
    nr, nc, nt = 120, 152, 14300
    cells = nr * nc
    stride = _round16((cells + 7) // 8 + 4 * cells)
    chunk = INFLATE_SCRATCH_BYTES // stride
    assert stride == int(lib().gf_float_planes_bytes(nr, nc) + 15) // 16 * 16
    assert (stride, chunk) == (75248, 14269) and nt * stride > INFLATE_SCRATCH_BYTES and chunk + 16 < nt < 2 * chunk
    codec = gridfour_amd.CodecFloatHip(level=6)
    ctx = codec.ctx
    rng = np.random.default_rng(152)
    ints = oracle.dem_tiles(oracle.DEM_SEED + 6, nr, nc, 4, 0, 5)
    tiles = np.stack([(ints[k].astype(np.float32) * np.float32(0.1) - np.float32(300.0)).view(np.uint32) for k in range(5)] +
                     [float_ref.random_bits(rng, nr, nc), float_ref.random_bits(rng, nr, nc), float_ref.chain_bits(nr, nc)])
    encoded = codec.encode_floats_batch(1, nr, nc, tiles.view(np.float32))

    def rc(p, out):
        return oracle.lib().gvo_codec_float_decode(nr, nc, oracle._p(p, oracle.C.c_uint8), p.size, oracle._p(out, oracle.C.c_uint32))
    packs = []
    for t, pk in enumerate(encoded):
        assert pk == oracle.codec_float_encode(1, nr, nc, tiles[t], level=6), t
        packs.append(_Pack("intact %d" % t, pk, _verdict(rc, cells, np.uint32, pk)))
        assert np.array_equal(packs[-1].verdict, tiles[t])
    noisy = 5                                                        # random bits: sign bits and plane bytes non-zero all over
    good = encoded[noisy]
    streams = float_ref.split(good)
    plane = [zlib.decompress(s) for s in streams]
    flipped = bytearray(good)
    flipped[-1] ^= 0x10

    def rebuilt(p, stream):
        ss = list(streams)
        ss[p] = stream
        return float_ref.frame(1, ss)
    damaged = [("adler", flipped), ("framing cut", good[:len(good) // 2]),
               ("ends early", rebuilt(3, streams[3][:len(streams[3]) // 2])),           # the stream itself runs out of input
               ("short sign", rebuilt(0, zlib.compress(plane[0][:len(plane[0]) // 3], 6))),
               ("empty sign", rebuilt(0, zlib.compress(b"", 6))),
               ("short exponent", rebuilt(1, zlib.compress(plane[1][:len(plane[1]) // 3], 6)))]
    for label, data in damaged:
        packs.append(_Pack(label, data, _verdict(rc, cells, np.uint32, data)))
    assert packs[_index(packs, "adler")].verdict is None and packs[_index(packs, "framing cut")].verdict is None
    for label in ("ends early", "short sign", "empty sign", "short exponent"):
        p = packs[_index(packs, label)]
        assert p.ok and not np.array_equal(p.verdict, tiles[noisy]), label
    placed = _seam_placements(packs, nt, chunk, ["intact 0", "intact 5", "intact 7", "intact 2"], ["adler", "short sign", "framing cut"])
    for i, label in ((5, "short sign"), (6, "empty sign"), (7, "short exponent"), (8, "ends early"), (9, "empty sign")):
        placed[i] = _index(packs, "intact %d" % (5 + i % 2))         # slot i of the plane scratch: random planes from chunk one
        placed[chunk + i] = _index(packs, label)
    seq = _sequence(20261, nt, chunk, packs, placed)

    def call(n, d_blob, blob_bytes, d_off, slot, d_len, d_val, d_st):
        check(lib().gf_float_decode_batch_f32_dev(ctx.handle, None, nr, nc, n, d_blob, blob_bytes, d_off, d_len, d_val, d_st),
              "gf_float_decode_batch_f32_dev")
    _run_offsets(ctx, call, cells, np.uint32, packs, seq, "float, %d tiles" % nt)
    # the grown scratch, full of the large call's planes, serves a later, small call
    small = [_index(packs, x) for x in ("empty sign", "intact 6", "adler", "short sign", "short exponent")]
    _run_offsets(ctx, call, cells, np.uint32, packs, np.array(small), "float, 5 tiles behind")


# ---- LSOP12 ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lsop_packs():
    """Canonical (type 2), legacy-Huffman (type 0) and Deflate (type 1) containers of 120 x 150 tiles, and damaged ones."""
    import gridfour_amd
    nr, nc = 120, 150
    cells = nr * nc
    codec = gridfour_amd.LsCodecHip(deflate_enabled=True)
    dem = oracle.dem_tiles(oracle.DEM_SEED + 4, nr, nc, 8, 0, 4)
    # (the Deflate container wins on the last three)
    tiles = np.stack([dem[0], dem[1], make_tile("smooth", nr, nc), make_tile("noise8", nr, nc), make_tile("steps", nr, nc),
                      make_tile("sparse_big", nr, nc), make_tile("sparse_big", nr, nc, seed=3)])
    encoded, types, est = codec.encode_batch(4, nr, nc, tiles)
    assert (est == 0).all() and list(types[:4]) == [2, 2, 2, 2] and list(types[4:]) == [1, 1, 1]

    def rc(p, out):
        return oracle.lib().gvo_lsop12_decode(nr, nc, oracle._p(p, oracle.C.c_uint8), p.size, oracle._p(out, oracle.C.c_int32))
    packs = []
    for t, pk in enumerate(encoded):
        ref, typ = oracle.lsop12_encode(4, nr, nc, tiles[t], True)
        assert bytes(pk) == ref and typ == types[t], t
        packs.append(_Pack("%s %d" % ("canon" if typ == 2 else "deflate", t), pk, _verdict(rc, cells, np.int32, pk)))
        assert np.array_equal(packs[-1].verdict, tiles[t])
    for t in (2, 3):
        pk = oracle.lsop12_encode_legacy_huffman(4, nr, nc, dem[t])
        packs.append(_Pack("legacy %d" % t, pk, _verdict(rc, cells, np.int32, pk)))
        assert np.array_equal(packs[-1].verdict, dem[t])
    big = bytes(encoded[5])
    second = bytearray(big)
    second[-1] ^= 0x10                                               # the Adler-32 of the second zlib stream
    first = bytearray(big)
    first[len(big) // 3] ^= 0x55                                     # inside the first
    canon = bytes(encoded[0])
    for label, data in (("deflate, second stream damaged", second), ("deflate, first stream damaged", first),
                        ("deflate cut", big[:len(big) // 2]), ("canon cut", canon[:len(canon) // 2]), ("header cut", canon[:40])):
        packs.append(_Pack(label, data, _verdict(rc, cells, np.int32, data)))
        assert packs[-1].verdict is None, label
    return nr, nc, codec.ctx, packs


@pytest.mark.parametrize("form", ["offsets", "slots"])
def test_lsop_batch_crosses_the_scratch_seam(lsop_packs, form):
    """gf_lsop12_decode_batch_i32_dev, 120 x 150: stride = roundUp(6 * (771 + 17,228) + 192, 16) = 108,192 bytes of scratch a tile,
    chunk = 384 MiB / 108,192 = 3,721 tiles; 3,760 tiles, canonical, legacy-Huffman and Deflate containers on both sides of the
    seam.  Once through d_offsets and once in slots (d_offsets = NULL): the chunk loop derives its view of the blob differently."""
    from gridfour_amd import DeviceBuffer as B, lib
    from gridfour_amd._lib import check
    nr, nc, ctx, packs = lsop_packs
    nt, cells = 3760, nr * nc
    n_init, n_int = 4 * nr + 2 * nc - 9, (nr - 2) * (nc - 4)
    stride = _round16(6 * (n_init + n_int) + 192)
    chunk = LSOP_INFLATE_SCRATCH_BYTES // stride
    assert (stride, chunk) == (108192, 3721) and nt * stride > LSOP_INFLATE_SCRATCH_BYTES and chunk + 8 < nt < 2 * chunk
    placed = _seam_placements(packs, nt, chunk, ["deflate 4", "canon 1", "deflate 5", "legacy 2"],
                              ["deflate, second stream damaged", "canon cut", "deflate, first stream damaged"])
    placed[chunk + 4] = _index(packs, "deflate 6")
    placed[chunk + 5] = _index(packs, "legacy 3")
    placed[chunk + 6] = _index(packs, "canon 3")
    seq = _sequence(20262, nt, chunk, packs, placed)
    for side in (seq[:chunk], seq[chunk:]):                          # every container type on both sides of the seam
        assert {packs[k].label.split()[0] for k in side} >= {"canon", "legacy", "deflate"}
    rs = _round16(int(lib().gf_lsop12_residual_count(nr, nc)))
    small = np.array([_index(packs, x) for x in ("deflate 5", "deflate, second stream damaged", "canon 0", "legacy 3", "deflate 4")])
    for which, sq in (("%d tiles" % nt, seq), ("5 tiles behind", small)):
        n = len(sq)
        where = "lsop %s, %s" % (form, which)
        blob, starts, lens = _small_blob(packs)
        if form == "slots":
            slot = _round16(int(lens.max()) + 16)
            table = np.zeros((len(packs), slot), np.uint8)
            for k, p in enumerate(packs):
                table[k, :len(p.data)] = np.frombuffer(p.data, np.uint8)
            blob = table[sq]                                         # the slots, one fancy-indexed assignment
            d_off = None
        else:
            slot = 0
            d_off = B(ctx, n * 8 + 16).upload(starts[sq])
        d_blob = B(ctx, blob.nbytes + 64).upload(blob)
        d_len = B(ctx, n * 4 + 16).upload(lens[sq])
        d_val = B(ctx, n * cells * 4 + GUARD).fill(SENTINEL)
        d_st = B(ctx, n * 4 + GUARD).fill(SENTINEL)
        d_res, d_co, d_sc = B(ctx, n * rs * 4 + 16), B(ctx, n * 64 + 16), B(ctx, n * 4 + 16)
        check(lib().gf_lsop12_decode_batch_i32_dev(ctx.handle, None, nr, nc, n, d_blob.ptr, blob.nbytes, d_off.ptr if d_off else None,
                                                   slot, d_len.ptr, d_val.ptr, d_st.ptr, d_res.ptr, rs, d_co.ptr, d_sc.ptr),
              "gf_lsop12_decode_batch_i32_dev")
        ctx.synchronize()
        vals = d_val.download(np.int32, n * cells).reshape(n, cells)
        st = d_st.download(np.int32, n)
        _guards(d_val, n * cells * 4, d_st, n, where)
        for b in (d_blob, d_off, d_len, d_val, d_st, d_res, d_co, d_sc):
            if b is not None:
                b.free()
        _check_tiles(packs, sq, vals, st, where)
