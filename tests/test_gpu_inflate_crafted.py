"""k_inflate (gvrs_inflate.hip) against the host's zlib on the hand-built catalogue of tests/deflate_craft.py: every rule of
inflate.c / inftrees.c by name -- whole streams at every input alignment, every byte prefix of every small stream (where zlib
waits and where it throws, for every field), every amount of room -- and through the three containers that carry Deflate,
against the oracle's decoders.  Byte-exact: a stream zlib accepts gives status 0, the same count and the same bytes; a stream
zlib rejects gives -1.  The one documented deviation: a preset-dictionary header (Z_NEED_DICT) is status 0 with nothing
produced, as java.util.zip.Inflater.inflate returns 0 with needsDictionary() set."""
import struct
import zlib

import numpy as np
import pytest

import deflate_craft as dc
import oracle
from test_gpu_inflate import _host, _inflate
from tilegen import make_tile

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def catalogue():
    return dc.cases()


def _room(c):
    return (len(c.expect) if isinstance(c.expect, bytes) else 0) + 64


def _is_need_dict(stream):
    try:
        zlib.decompressobj().decompress(stream)
    except zlib.error as e:
        return not any(m in str(e) for m in dc.MESSAGES)
    return False


def _compare(names, streams, caps, residues):
    """one launch; every stream against _host.  Returns (accepted, rejected, need_dict): how many were compared with each verdict."""
    outs, prod, st = _inflate(streams, caps, residues=residues, odd_out=True)
    n_ok = n_err = n_dict = 0
    for i, s in enumerate(streams):
        want, err = _host(s, caps[i])
        where = (names[i], len(s), int(caps[i]), int(residues[i]), int(st[i]), int(prod[i]))
        if err and names[i] == "valid/preset_dictionary_header" and _is_need_dict(s):
            assert st[i] == 0 and prod[i] == 0, where
            n_dict += 1
        elif err:
            assert st[i] == -1, where
            n_err += 1
        else:
            assert st[i] == 0 and prod[i] == len(want) and outs[i] == want, where + (len(want),)
            n_ok += 1
    return n_ok, n_err, n_dict


def test_whole_streams_at_every_input_alignment(catalogue):
    names, streams, caps, res = [], [], [], []
    for c in catalogue:
        for r in range(4):
            names.append(c.name)
            streams.append(c.stream)
            caps.append(_room(c))
            res.append(r)
    n_ok, n_err, n_dict = _compare(names, streams, caps, res)
    kinds = [c.kind for c in catalogue]
    assert n_ok + n_err + n_dict == 4 * len(catalogue)
    assert n_ok == 4 * (kinds.count("valid") + kinds.count("ended")) > 0
    assert n_err == 4 * kinds.count("reject") > 0 and n_dict == 4


def test_every_prefix_of_every_small_stream(catalogue):
    names, streams, caps, res = [], [], [], []
    small = [c for c in catalogue if len(c.stream) <= 160]
    for c in small:
        for cut in range(len(c.stream) + 1):
            names.append(c.name)
            streams.append(c.stream[:cut])
            caps.append(_room(c))
            res.append((cut + len(names)) & 3)
    assert len(small) >= 300 and len(streams) == sum(len(c.stream) + 1 for c in small) > 10000
    n_ok, n_err, n_dict = _compare(names, streams, caps, res)
    assert n_ok + n_err + n_dict == len(streams)
    # every rejecting small stream is rejected whole, and waits or is accepted at length 0
    assert n_err >= sum(c.kind == "reject" for c in small) > 0 and n_ok > len(small) and n_dict > 0


def test_every_room(catalogue):
    names, streams, caps = [], [], []
    n_small = n_large = 0
    for c in catalogue:
        if c.kind != "valid":
            continue
        n = len(c.expect)
        if n <= 300:
            rooms = range(0, n + 2)
            n_small += 1
        else:
            rooms = {0, 1, 1023, 1024, 1025, n - 1, n, n + 1}
            for s in dc.MATCH_STARTS[c.name]:
                rooms |= {s - 1, s, s + 1}
            rooms = sorted(rooms)
            n_large += 1
        for cap in rooms:
            names.append(c.name)
            streams.append(c.stream)
            caps.append(cap)
    assert n_small == 6 and n_large == 13
    # a match that reaches too far back, arriving exactly when the room is used up: zlib looks at the room first, no error;
    # with one byte more it is an error
    by_name = {c.name: c for c in catalogue}
    for name, at in dc.TOO_FAR_BACK_AT.items():
        for cap in (at, at + 1):
            names.append(name)
            streams.append(by_name[name].stream)
            caps.append(cap)
    assert _host(by_name["reject/too_far_back_at_position_1"].stream, 1) == (b"a", 0)
    assert _host(by_name["reject/too_far_back_at_position_1"].stream, 2) == (None, -1)
    n_ok, n_err, n_dict = _compare(names, streams, caps, [i & 3 for i in range(len(streams))])
    assert n_ok + n_err == len(streams) and n_dict == 0
    assert n_err == 3 and n_ok == len(streams) - 3 > 1000


# ---- through the containers, against the oracle's decoders -------------------------------------------------------------
HOWS = ("stored", "fixed", "dyn_literals", "dyn15", "mixed")


def deflate_packings(nr=12, nc=40):
    """CodecDeflate packings (10-byte header, one zlib stream of the M32 bytes) of one tile with the stream rebuilt five ways"""
    v = make_tile("smooth", nr, nc, seed=5)
    good, _ = oracle.codec_deflate_encode(2, nr, nc, v)
    m32 = zlib.decompress(good[10:])
    assert struct.unpack_from("<I", good, 6)[0] == len(m32)
    return v, [good] + [good[:10] + dc.compress(m32, how)[0] for how in HOWS]


def float_packings(nr=9, nc=14):
    """CodecFloat packings (two header bytes, five length-prefixed zlib streams) with every plane rebuilt five ways"""
    rng = np.random.default_rng(77)
    f = (np.sin(np.arange(nr * nc) / 5.0) * 300.0 + rng.standard_normal(nr * nc)).astype(np.float32)
    good = oracle.codec_float_encode(3, nr, nc, f.view(np.uint32), 6)
    planes, off = [], 2
    for _ in range(5):
        zn = struct.unpack_from("<I", good, off)[0]
        planes.append(zlib.decompress(good[off + 4:off + 4 + zn]))
        off += 4 + zn
    assert off == len(good)
    packs = [good]
    for k in range(len(HOWS)):
        pk = good[:2]
        for p, plane in enumerate(planes):
            z = dc.compress(plane, HOWS[(k + p) % len(HOWS)])[0]          # every plane of a packing another way
            pk += struct.pack("<I", len(z)) + z
        packs.append(pk)
    return f, packs


def lsop_packings(nr=20, nc=24):
    """LSOP12 type-1 containers (header, TWO zlib streams back to back: the second begins where the first one's inflater
    stopped reading) with the first stream's last block -- stored, fixed or dynamic -- ending at each of the eight bit phases.
    Returns (cells, packings, phases: the (kind of last block, bit phase) of each rebuilt packing)."""
    y, x = np.mgrid[0:nr, 0:nc]
    v = (3 * x + 5 * y + 40 * ((x // 8 + y // 8) % 2)).astype(np.int32).ravel()
    good, typ = oracle.lsop12_encode(1, nr, nc, v, True)
    assert typ == 1 and good[1] & 0x40 and not good[1] & 0x80              # revised header, no value checksum
    o = 2 + 53 + 8
    n1, n2 = struct.unpack_from("<II", good, 2 + 53)
    d = zlib.decompressobj()
    m1 = d.decompress(good[o:])
    m2 = zlib.decompress(d.unused_data)
    assert d.eof and len(m1) == n1 and len(m2) == n2
    packs, phases = [good], []
    for last in ("stored", "fixed", "dyn_literals", "dyn15"):
        for k in range(8):
            z1, phase = dc.compress(m1, ["fixed", last], phase_blocks=k)
            z2 = dc.compress(m2, HOWS[k % len(HOWS)])[0]
            packs.append(good[:o] + z1 + z2)
            phases.append((last, phase))
    return v, packs, phases


def test_crafted_streams_inside_deflate_packings():
    import gridfour_amd
    nr, nc = 12, 40
    v, packs = deflate_packings(nr, nc)
    vals, st = gridfour_amd.CodecDeflateHip().decode_batch(nr, nc, packs)
    assert len(packs) == 1 + len(HOWS)
    for k, pk in enumerate(packs):
        want = oracle.codec_deflate_decode(nr, nc, pk)
        assert np.array_equal(want, v.ravel()), k
        assert st[k] == 0 and np.array_equal(vals[k], want), (k, int(st[k]))


def test_crafted_streams_inside_float_packings():
    import gridfour_amd
    nr, nc = 9, 14
    f, packs = float_packings(nr, nc)
    vals, st = gridfour_amd.CodecFloatHip(level=6).decode_floats_batch(nr, nc, packs)
    assert len(packs) == 1 + len(HOWS)
    for k, pk in enumerate(packs):
        want = oracle.codec_float_decode(nr, nc, pk)
        assert np.array_equal(want, f.view(np.uint32)), k
        assert st[k] == 0 and np.array_equal(vals[k].view(np.uint32), want), (k, int(st[k]))


def test_second_lsop_stream_is_found_behind_every_end_phase_of_the_first():
    import gridfour_amd
    nr, nc = 20, 24
    v, packs, phases = lsop_packings(nr, nc)
    assert {p for last, p in phases if last == "stored"} == {0}
    for last in ("fixed", "dyn_literals", "dyn15"):
        assert {p for k, p in phases if k == last} == set(range(8)), last
    vals, st = gridfour_amd.LsCodecHip().decode_batch(nr, nc, packs)
    assert len(packs) == 1 + 4 * 8
    for k, pk in enumerate(packs):
        want = oracle.lsop12_decode(nr, nc, pk)
        assert np.array_equal(want, v), k
        assert st[k] == 0 and np.array_equal(vals[k], want), (k, int(st[k]), phases[k - 1] if k else None)
