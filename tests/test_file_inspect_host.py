"""CPU-only: gf_file_inspect, the host form of the inspector, against the sequential restatement (tests/gvrs_inspect_ref.py) on the
reference's sample files and on every image of tests/inspect_cases.py, field for field; its capacity rules and refusals."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import gvrs_inspect_ref as R
import inspect_cases as K
from gridfour_amd import GvrsFileHip, GvrsHipError, _lib
from gridfour_amd.codec import _FILE_INSPECT_REPORT, _ptr

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLES = sorted(glob.glob(os.path.join(HERE, "golden", "ref_samples", "*.gvrs")))


def test_samples_equal_the_restatement():
    assert len(SAMPLES) == 15
    for path in SAMPLES:
        f = GvrsFileHip(path)
        got = f.inspect()
        assert R.same(got, R.inspect(f.image.tobytes(), R.facts_of(f))) == [] and got.passed and got.guards_intact, path


def test_cases_equal_the_restatement():
    for name, image in K.all_cases().items():
        f = GvrsFileHip(image)
        got = f.inspect()
        assert R.same(got, R.inspect(image, R.facts_of(f))) == [], name
        assert got.guards_intact and got.stop_name is not None, name


def test_another_image_than_the_opened_one():
    """the header is the opened file's; the bytes behind it are judged as they are, every truncation on the 8-byte grid included"""
    image = K.all_cases()["sound: shuffled"]
    f = GvrsFileHip(image)
    facts = R.facts_of(f)
    other = K.all_cases()["damaged: tile and metadata"]
    assert R.same(f.inspect(other), R.inspect(other, facts)) == []
    for n in list(range(facts["content_pos"], facts["content_pos"] + 200)) + list(range(len(image) - 300, len(image))):
        assert R.same(f.inspect(image[:n]), R.inspect(image[:n], facts)) == [], n


def test_capacity_of_the_record_list():
    image = K.all_cases()["damaged: a good record between"]
    f = GvrsFileHip(image)
    whole = f.inspect()
    n = whole.n_records
    for cap in (0, 1, n - 1):
        rc, got = f.inspect(records_cap=cap, bad_cap=8, return_code=True)
        assert rc == _lib.ERR_CAPACITY and got.status == _lib.ERR_CAPACITY and got.n_records == n and got.guards_intact, cap
    rc, got = f.inspect(records_cap=n, bad_cap=8, return_code=True)
    assert rc == 0 and got.records == whole.records and got.guards_intact
    with pytest.raises(GvrsHipError):
        f.inspect(records_cap=n - 1)


def test_capacity_of_the_bad_tiles():
    image = K.all_cases()["damaged: a good record between"]
    f = GvrsFileHip(image)
    whole = f.inspect()
    assert whole.n_bad_tiles == 2 and len(whole.bad_tiles) == 2
    for cap in (0, 1, 2, 5):
        got = f.inspect(bad_cap=cap)
        assert got.n_bad_tiles == 2 and got.bad_tiles == whole.bad_tiles[:cap] and got.guards_intact, cap


def test_without_a_record_list():
    image = K.all_cases()["damaged: tile and tile"]
    f = GvrsFileHip(image)
    report = np.zeros(1, _FILE_INSPECT_REPORT)
    assert _lib.lib().gf_file_inspect(f._h, _ptr(f.image), f.image.size, _ptr(report), None, 0, None, 0) == 0
    want = R.inspect(image, R.facts_of(f))
    assert int(report[0]["n_records"]) == want["n_records"] and int(report[0]["n_bad_tiles"]) == 2 and int(report[0]["stop"]) == R.TWO_CHECKSUM_FAILURES


def test_refusals():
    image = K.all_cases()["sound: compact"]
    f = GvrsFileHip(image)
    L = _lib.lib()
    report = np.zeros(1, _FILE_INSPECT_REPORT)
    bad = np.zeros(4, np.int32)
    assert L.gf_file_inspect(None, _ptr(f.image), f.image.size, _ptr(report), _ptr(bad), 4, None, 0) == _lib.ERR_ARG
    assert L.gf_file_inspect(f._h, None, f.image.size, _ptr(report), _ptr(bad), 4, None, 0) == _lib.ERR_ARG
    assert L.gf_file_inspect(f._h, _ptr(f.image), f.image.size, None, _ptr(bad), 4, None, 0) == _lib.ERR_ARG
    assert L.gf_file_inspect(f._h, _ptr(f.image), f.image.size, _ptr(report), None, 4, None, 0) == _lib.ERR_ARG
    assert L.gf_file_inspect(f._h, _ptr(f.image), f.info["content_pos"] - 1, _ptr(report), _ptr(bad), 4, None, 0) == _lib.ERR_ARG
    other = GvrsFileHip(SAMPLES[0])                                # (another header record size: not the image that was opened)
    assert other.info["content_pos"] != f.info["content_pos"]
    assert L.gf_file_inspect(other._h, _ptr(f.image), f.image.size, _ptr(report), _ptr(bad), 4, None, 0) == _lib.ERR_ARG
    assert L.gf_file_inspect_plan(None, 100, None, None, None) == _lib.ERR_ARG
    seg, chunk, most = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.gf_file_inspect_plan(f._h, f.image.size, C.byref(seg), C.byref(chunk), C.byref(most)) == 0
    assert seg.value % 8 == 0 and seg.value >= 8 and chunk.value % 256 == 0 and most.value >= f.inspect().n_records
    assert L.gf_file_inspect_plan(f._h, f.image.size, None, None, None) == 0
    # the content position alone is a clean end with no record
    got = f.inspect(image[:f.info["content_pos"]])
    assert (got.n_records, got.complete, got.failed, got.termination_pos, got.tile_dir_passed) == (0, 1, 0, f.info["content_pos"], 0)
