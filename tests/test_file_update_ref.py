"""The model of an in-place update (tests/gvrs_file_update_ref.py) held to its own checks, on the CPU: opening and closing a
reference file changes nothing, and every scenario of tests/file_update_cases.py takes the allocator's case it is named for
and leaves a file whose records tile it, whose list is the free records, and which gf_file_open opens."""
import glob
import os
import struct

import pytest

import file_update_cases as U
import gvrs_file_update_ref as R
from gridfour_amd import GvrsFileHip

SAMPLES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_samples", "*.gvrs")))


def test_there_are_fifteen_samples():
    assert len(SAMPLES) == 15


@pytest.mark.parametrize("path", SAMPLES, ids=os.path.basename)
def test_open_and_close_returns_the_reference_file(path):
    data = open(path, "rb").read()
    f = GvrsFileHip(data)
    out, opened, final, _, closing = R.ref_update(data, -(-f.grid[1] // f.grid[3]), bool(f.info["codec_ids"]), [], [],
                                                  struct.unpack_from("<q", data, 40)[0])
    assert out == data and final == []
    assert len(opened) == 1                                       # the freed directories merged into one node ...
    assert [e[1] for e in closing] == (["split", "exact"] if f.info["metadata_dir_pos"] else ["exact"])   # ... and land where they were


@pytest.mark.parametrize("checksums", [True, False], ids=["crc", "nocrc"])
@pytest.mark.parametrize("name", sorted(U.SCENARIOS))
def test_scenario_takes_its_case_and_keeps_the_invariants(name, checksums):
    image, records, tiles, status, flags, compression, wanted = U.scenario(name, checksums)
    out, opened, final, writes, _ = U.model(image, records, tiles, status, flags, compression)
    assert U.holds(writes, wanted), writes
    U.check_invariants(out, final)
    f = GvrsFileHip(out)
    assert f.info["freespace_dir_pos"] == struct.unpack_from("<q", out, 56)[0]
    for k, (r, t) in enumerate(zip(records, tiles)):
        if status is not None and status[k] < 0:
            assert f.tile_position(t) == GvrsFileHip(image).tile_position(t)
        elif r:
            p = f.tile_position(t)
            assert out[p - 8:p - 8 + len(r)] == r
        else:
            assert f.tile_position(t) == 0


def test_the_three_orders_give_three_layouts():
    outs = set()
    for name in ("row-major", "reversed", "permuted"):
        image, records, tiles, *_ = U.scenario(name)
        outs.add(U.model(image, records, tiles)[0])
    assert len(outs) == 3


def test_no_node_fits_leaves_the_trailing_node():
    image, records, tiles, *_ = U.scenario("no node fits")
    out, opened, final, writes, _ = U.model(image, records, tiles)
    assert 8 <= opened[-1][1] - len(records[0]) <= 24 and opened[-1][0] + opened[-1][1] == len(image)
    assert writes[-1][:3] == ("alloc", "append", len(image))


def test_a_second_update_of_the_updated_image():
    image, records, tiles, *_ = U.scenario("replace frees first")
    once, _, final, _, _ = U.model(image, records, tiles)
    assert len(final) >= 2
    records2, tiles2 = U.writes_of([(0, 0), (60, 32), (2, 0), (61, 400)], seed=5)
    twice, opened, final2, writes, _ = U.model(once, records2, tiles2)
    assert len(opened) >= 2
    U.check_invariants(twice, final2)
    GvrsFileHip(twice)
