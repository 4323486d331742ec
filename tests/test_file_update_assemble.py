"""gf_file_update_begin / _free_list / _plan / _assemble against the model of tests/gvrs_file_update_ref.py, byte for byte, on
the CPU: every scenario of tests/file_update_cases.py with and without checksums, the free-space directory's cases, all or
nothing, the refusals of a damaged image, a second update."""
import struct

import numpy as np
import pytest

import file_update_cases as U
import gvrs_file_build as B
from gridfour_amd import GvrsFileHip, GvrsHipError, _lib

CRC = pytest.mark.parametrize("checksums", [True, False], ids=["crc", "nocrc"])


def lib_update(image, records, tiles, status=None, flags=0, **kw):
    f = GvrsFileHip(image)
    u = f.update_begin()
    try:
        return f.update_assemble(u, records, tiles, U.TIME, status, flags, **kw), u.free_list
    finally:
        u.end()
        f.close()


def both(image, records, tiles, status=None, flags=0, compression=True):
    want, opened, final, writes, closing = U.model(image, records, tiles, status, flags, compression)
    got, lib_opened = lib_update(image, records, tiles, status, flags)
    assert lib_opened == opened
    assert got == want
    U.check_invariants(got, final)
    return got, final, writes, closing


@CRC
@pytest.mark.parametrize("name", sorted(U.SCENARIOS))
def test_scenario_equals_the_model(name, checksums):
    image, records, tiles, status, flags, compression, _ = U.scenario(name, checksums)
    both(image, records, tiles, status, flags, compression)


@pytest.mark.parametrize("extended", [False, True], ids=["compact", "extended"])
def test_directory_of_more_than_64_chunks(tmp_path_factory, extended):
    """The shape at which the device's fold gives a lane a second chunk (tests/dir_seams.py), on the host: a grid of one row of n
    tiles, a file with tile 0 alone, tile 0 written anew and the last tile written, against the model"""
    from dir_seams import SEAMS, read_chunk
    n = dict(SEAMS)["65C+1"](read_chunk(tmp_path_factory), 8 if extended else 4)
    image = U.make_file([("t", 0, 40)], grid=(2, 2 * n, 2, 2))
    records, tiles = U.writes_of([(0, 48), (n - 1, 24)])
    want, opened, final, _, _ = U.model(image, records, tiles, flags=int(extended), n_tile_cols=n)
    got, lib_opened = lib_update(image, records, tiles, None, int(extended))
    assert lib_opened == opened and got == want
    U.check_invariants(got, final, n_tile_cols=n)
    td = struct.unpack_from("<q", got, 80)[0]
    assert struct.unpack_from("<iiii", got, td + 8) == (0, 0, 1, n) and got[td + 1] == int(extended)


def test_the_deviation_keeps_the_tile():
    """the reference would write the standard form into the block it freed and lose the entry: here the record is allocated"""
    image, records, tiles, *_ = U.scenario("the deviation")
    got, _, _, _ = both(image, records, tiles)
    p = GvrsFileHip(got).tile_position(3)
    assert p == GvrsFileHip(image).tile_position(3) and got[p - 8:p - 8 + 72] == records[0]


@CRC
def test_free_space_directory_cases(checksums):
    # the old file has one (U.BASE), freed first at opening; the allocation of the new one consumes no node: it splits one
    image = U.make_file(U.BASE, checksums)
    got, final, _, closing = both(image, *U.writes_of([(3, 0)], checksums))
    assert closing[-1][1] == "split" and struct.unpack_from("<i", got, struct.unpack_from("<q", got, 56)[0])[0] == len(final)
    # the allocation consumes a node (an exact fit): the count is one less and the record 12 bytes roomier.  Four nodes need a
    # record of 64 bytes; the old file's hole of 64 is the first that fits.
    layout = [("t", 0, 40), ("f", 64), ("t", 1, 48), ("t", 2, 24), ("t", 3, 56), ("t", 4, 24), ("t", 5, 40)]
    image = U.make_file(layout, checksums)
    got, final, _, closing = both(image, *U.writes_of([(2, 0), (4, 0)], checksums))
    fs = struct.unpack_from("<q", got, 56)[0]
    assert closing[-1][1] == "exact" and len(final) == 3 and struct.unpack_from("<ii", got, fs - 8) == (64, 3)
    assert struct.unpack_from("<i", got, fs)[0] == 3 and 4 + 12 * 3 + 12 <= 64 - 12
    # the final list is empty: the word is 0 and there is no record (a file without nodes, nothing freed)
    image = U.make_file([("t", 0, 40), ("t", 1, 48)], checksums)
    got, final, _, _ = both(image, *U.writes_of([(7, 64)], checksums))
    assert final == [] and struct.unpack_from("<q", got, 56)[0] == 0
    # an old free-space directory record that is 12 bytes roomier than its count needs
    image = U.make_file(U.BASE, checksums, free_dir_slack=1)
    both(image, *U.writes_of([(50, 64)], checksums))


@CRC
def test_a_second_update(checksums):
    image, records, tiles, *_ = U.scenario("replace frees first", checksums)
    once, final, _, _ = both(image, records, tiles)
    assert len(final) >= 2
    twice, _, _, _ = both(once, *U.writes_of([(0, 0), (60, 32), (2, 0), (61, 400)], checksums, seed=5))
    both(twice, *U.writes_of([(61, 0), (62, 24)], checksums, seed=6))


def test_three_orders_three_layouts():
    outs = {both(*U.scenario(name)[:3])[0] for name in ("row-major", "reversed", "permuted")}
    assert len(outs) == 3


def test_all_or_nothing():
    image, records, tiles, *_ = U.scenario("trailing node too small")
    want = U.model(image, records, tiles)[0]
    f = GvrsFileHip(image)
    u = f.update_begin()
    rc, buf, need = f.update_assemble(u, records, tiles, U.TIME, image_cap=len(want) - 8, return_code=True)
    assert rc == _lib.ERR_CAPACITY and need == len(want)
    assert buf[:len(image)] == image and set(buf[len(image):]) <= {0xA5}
    rc, buf, need = f.update_assemble(u, records, tiles, U.TIME, image_cap=len(want), return_code=True)
    assert rc == 0 and need == len(want) and buf == want
    assert u.plan()[0] >= len(want) and u.plan((0, 0, 2, 2))[1] == len(u.free_list) + 1 + 3


def test_refused_records_change_nothing():
    image, records, tiles, *_ = U.scenario("exact fit")
    f = GvrsFileHip(image)
    u = f.update_begin()
    cap = u.plan()[0]
    bad = [([records[0], records[0]], [50, 50]), ([records[0]], [100]), ([records[0]], [-1]), ([records[0][:-4]], [50]), ([records[0][:16]], [50])]
    for recs, idx in bad:
        rc, buf, _ = f.update_assemble(u, recs, idx, U.TIME, image_cap=cap, return_code=True)
        assert rc == _lib.ERR_ARG and buf[:len(image)] == image and set(buf[len(image):]) <= {0xA5}
    rc, buf, _ = f.update_assemble(u, records, tiles, U.TIME, image_cap=len(image) - 8, return_code=True)
    assert rc == _lib.ERR_ARG
    # an old record whose size word is damaged: the verdict, and nothing written
    p = f.tile_position(2)
    hurt = bytearray(image)
    struct.pack_into("<i", hurt, p - 8, 60)
    u2 = f.update_begin(bytes(hurt))
    r2, t2 = U.writes_of([(2, 64)])
    buf0 = np.full(cap, 0xA5, np.uint8)
    buf0[:len(hurt)] = np.frombuffer(bytes(hurt), np.uint8)
    rc, buf, _ = f.update_assemble(u2, r2, t2, U.TIME, image_cap=cap, return_code=True)
    assert rc == _lib.ERR_FORMAT and buf == buf0.tobytes()


def refused(f, image):
    try:
        u = f.update_begin(image)
    except GvrsHipError as e:
        return e.status
    u.end()
    return 0


def test_each_rule_of_begin():
    image = U.make_file(U.BASE)
    f = GvrsFileHip(image)
    fs = struct.unpack_from("<q", image, 56)[0]
    td = struct.unpack_from("<q", image, 80)[0]
    node0, size0 = struct.unpack_from("<qi", image, fs + 4)
    node1, _ = struct.unpack_from("<qi", image, fs + 16)

    def patched(at, fmt, *v, crc_of=None):
        b = bytearray(image)
        struct.pack_into(fmt, b, at, *v)
        return bytes(b)

    F, Bd = _lib.ERR_FORMAT, _lib.ERR_BOUNDS
    cases = {
        "nodes descend": (patched(fs + 4, "<qiqi", node1, 96, node0, 64), F),
        "nodes overlap": (patched(fs + 16, "<q", node0 + 32), F),
        "nodes touch": (patched(fs + 16, "<q", node0 + size0), F),
        "position no multiple of 8": (patched(fs + 4, "<q", node0 + 4), F),
        "size no multiple of 8": (patched(fs + 12, "<i", 60), F),
        "size below 24": (patched(fs + 12, "<i", 16), F),
        "node in front of the content": (patched(fs + 4, "<q", 64), F),
        "node behind the image": (patched(fs + 28, "<q", len(image) + 64), Bd),
        "node's head states another size": (patched(node0, "<i", 56), F),
        "node's head has another type": (patched(node0 + 4, "<i", 2), F),
        "free-space directory's type": (patched(fs - 4, "<i", 4), F),
        "free-space directory's size": (patched(fs - 8, "<i", 60), F),
        "free-space directory runs past the image": (patched(fs - 8, "<i", 4096), Bd),
        "count the record cannot hold": (patched(fs, "<i", 4), F),
        "negative count": (patched(fs, "<i", -1), F),
        "tile directory's type": (patched(td - 4, "<i", 2), F),
        "tile directory's size": (patched(td - 8, "<i", 100), F),
        "tile directory too small for its entries": (patched(td - 8, "<i", 48), F),
        "a length that is no multiple of 8": (image + b"\0" * 4, F),
    }
    assert refused(f, image) == 0
    for name, (hurt, code) in cases.items():
        assert refused(f, hurt) == code, name
    # the metadata directory: a sample file has one
    import glob, os
    path = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_samples", "*.gvrs")))[0]
    data = open(path, "rb").read()
    g = GvrsFileHip(data)
    md = g.info["metadata_dir_pos"]
    assert md and refused(g, data) == 0
    b = bytearray(data)
    b[md - 4] = 5
    assert refused(g, bytes(b)) == F
    b = bytearray(data)
    struct.pack_into("<i", b, md - 8, 1 << 20)
    assert refused(g, bytes(b)) == Bd
    # another header record than the opened one's
    assert refused(g, image) == _lib.ERR_ARG


def test_every_prefix_of_an_image_with_a_free_space_directory():
    image = U.make_file(U.BASE)
    f = GvrsFileHip(image)
    content = f.info["content_pos"]
    ok = 0
    for n in range(content, len(image) + 1):
        try:
            u = f.update_begin(image[:n])
        except GvrsHipError as e:
            assert e.status in (_lib.ERR_FORMAT, _lib.ERR_BOUNDS, _lib.ERR_ARG)
            continue
        ok += 1
        nodes = u.free_list
        u.end()
        for (p, z), (q, _) in zip(nodes, nodes[1:]):
            assert p + z < q
        assert all(p % 8 == 0 and z % 8 == 0 and z >= 24 and p >= content and p + z <= n for p, z in nodes)
    assert ok == 1                                                 # the whole image alone
