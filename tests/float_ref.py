"""CodecFloat.encodeFloats / decodeFloats restated in plain numpy, from the Java text (compress/CodecFloat.java:300-325 the
delta rule, :328-392 the encoder, :395-458 the decoder).  Independent of oracle/: tests/test_float_ref.py pins the two against
each other at the shapes the GPU tests use, so that those compare the kernels with a reference that is itself checked there.

Cells are raw IEEE-754 bit patterns (uint32, row-major); bytes are taken modulo 256 throughout, which is what Java's
`(byte)` casts come to.
"""
import struct
import zlib

import numpy as np


def encode_deltas(plane, n_rows, n_cols):
    """encodeDeltas :300-313: every byte minus its left neighbour; the first cell of a row minus the first cell of the row
    before (the value as it was, not its delta); cell (0,0) minus 0."""
    p = np.asarray(plane, np.uint8).reshape(n_rows, n_cols)
    prior = np.zeros_like(p)
    prior[:, 1:] = p[:, :-1]
    prior[1:, 0] = p[:-1, 0]
    return (p - prior).ravel()                           # uint8 arithmetic wraps like (byte)


def decode_deltas(scratch, n_rows, n_cols):
    """decodeDeltas :315-325, in place in the reference: running sums along a row; the next row starts from the DECODED first
    cell of the row it follows."""
    d = np.asarray(scratch, np.uint8).reshape(n_rows, n_cols).astype(np.uint32)
    d[:, 0] = np.cumsum(d[:, 0])                         # the column-0 chain
    return (np.cumsum(d, axis=1) & 0xff).astype(np.uint8).ravel()


def planes(n_rows, n_cols, raw_bits):
    """The five byte planes the encoder hands to Deflater, in packing order: sign bits (LSB first), exponent, and the three
    mantissa planes (7, 8, 8 bits), each delta coded."""
    c = np.ascontiguousarray(raw_bits, np.uint32).ravel()
    assert c.size == n_rows * n_cols
    sign = np.packbits((c >> 31).astype(np.uint8), bitorder="little")
    exp = ((c >> 23) & 0xff).astype(np.uint8)
    m1 = encode_deltas(((c >> 16) & 0x7f).astype(np.uint8), n_rows, n_cols)
    m2 = encode_deltas(((c >> 8) & 0xff).astype(np.uint8), n_rows, n_cols)
    m3 = encode_deltas((c & 0xff).astype(np.uint8), n_rows, n_cols)
    return [sign, exp, m1, m2, m3]


def _deflate(data, level):
    """doDeflate :268-283: one complete zlib stream, written into byte[input.length + 128]."""
    return zlib.compress(bytes(data), level)[:len(data) + 128]


def frame(codec_index, streams):
    """:377-391: codec index, a zero, then five times [int32 LE length][stream]."""
    return bytes([codec_index & 0xff, 0]) + b"".join(struct.pack("<I", len(s)) + bytes(s) for s in streams)


def encode_floats(codec_index, n_rows, n_cols, raw_bits, level=9):
    return frame(codec_index, [_deflate(p.tobytes(), level) for p in planes(n_rows, n_cols, raw_bits)])


def split(packing):
    """The five zlib streams of a packing.  IOError where the framing runs off the packing (the reference dies of an
    ArrayIndexOutOfBoundsException there)."""
    streams, off = [], 2
    for _ in range(5):
        if off + 4 > len(packing):
            raise IOError("framing runs off the packing")
        n = struct.unpack_from("<i", packing, off)[0]
        off += 4
        if n < 0 or off + n > len(packing):
            raise IOError("framing runs off the packing")
        streams.append(bytes(packing[off:off + n]))
        off += n
    return streams


def _inflate_into(scratch, stream, room):
    """doInflate :285-298: a fresh Inflater, ONE inflate call with `room` bytes of output.  A stream that ends early gives what
    it has and no error; one that holds more is cut at the room; what is not written stays as it was."""
    try:
        out = zlib.decompressobj().decompress(stream, room)
    except zlib.error as e:
        raise IOError("Inflate failed: %s" % e)
    scratch[:len(out)] = np.frombuffer(out, np.uint8)
    return len(out)


def decode_floats(n_rows, n_cols, packing):
    """decodeFloats :395-458 -> raw bits.  ONE scratch array serves the five planes and the mantissa deltas are decoded in place:
    behind a short plane lies what the plane before left there."""
    n = n_rows * n_cols
    n_sign = (n + 7) // 8
    s = split(packing)
    scratch = np.zeros(n, np.uint8)
    _inflate_into(scratch, s[0], n_sign)
    raw = np.unpackbits(scratch[:n_sign], bitorder="little")[:n].astype(np.uint32) << 31
    _inflate_into(scratch, s[1], n)
    raw |= scratch.astype(np.uint32) << 23
    for k, (mask, shift) in enumerate(((0x7f, 16), (0xff, 8), (0xff, 0))):
        _inflate_into(scratch, s[2 + k], n)
        scratch[:] = decode_deltas(scratch, n_rows, n_cols)
        raw |= (scratch.astype(np.uint32) & mask) << shift
    return raw


# ---- what the tests feed it --------------------------------------------------------------------------------------------------

def random_bits(rng, n_rows, n_cols):
    """Full-random 32-bit cell patterns: every byte sum of the delta decoding wraps."""
    return rng.integers(0, 2 ** 32, n_rows * n_cols, dtype=np.uint64).astype(np.uint32)


def chain_bits(n_rows, n_cols):
    """A tile whose column-0 cell in row r has mantissa (r & 0x7f) << 16 | (r & 0xff) << 8 | (r * 3 & 0xff): every link of the
    column-0 chain is non-zero in all three planes, so a carry dropped at some row shows in every row behind it.  The other
    columns count on from there; signs and exponents vary with the row."""
    r = np.arange(n_rows, dtype=np.uint32)[:, None]
    c = np.arange(n_cols, dtype=np.uint32)[None, :]
    m0 = ((r & 0x7f) << 16) | ((r & 0xff) << 8) | ((r * 3) & 0xff)
    mant = (m0 + c * 0x010305) & 0x7fffff
    return ((((r + c) & 1) << 31) | (((r * 5 + c) & 0xff) << 23) | mant).astype(np.uint32).ravel()


def damaged_plane_packings(packing, level=6, long_by=100):
    """(short, long): packings rebuilt around `packing` with one plane's stream re-compressed from its first
    keep in {0, 1, len // 3, len - 1} bytes, for each of the five planes, plus one with two planes short at once; and packings in
    which one plane's stream carries `long_by` bytes more than the plane.  All are valid zlib streams: the reference decodes
    every one without an exception."""
    streams = split(packing)
    pl = [zlib.decompress(s) for s in streams]
    short = []
    for p in range(5):
        for keep in (0, 1, len(pl[p]) // 3, len(pl[p]) - 1):
            ss = list(streams)
            ss[p] = zlib.compress(pl[p][:keep], level)
            short.append(frame(packing[0], ss))
    ss = list(streams)
    ss[2] = zlib.compress(pl[2][:len(pl[2]) // 4], level)
    ss[4] = zlib.compress(pl[4][:7 % len(pl[4])], level)
    short.append(frame(packing[0], ss))
    rng = np.random.default_rng(len(packing))
    long = []
    for p in range(5):
        ss = list(streams)
        ss[p] = zlib.compress(pl[p] + rng.integers(1, 256, long_by).astype(np.uint8).tobytes(), level)
        long.append(frame(packing[0], ss))
    return short, long
