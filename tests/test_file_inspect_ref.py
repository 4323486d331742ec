"""CPU-only: tests/gvrs_inspect_ref.py, the sequential restatement of GvrsInspector, on the reference's own sample files and on
the images of tests/inspect_cases.py -- what each case must answer is stated here, from the reference's lines and the
deviations, before any library code is compared against the restatement."""
import glob
import os

import pytest

import gvrs_inspect_ref as R
import gvrs_walk
import inspect_cases as K
from gridfour_amd import GvrsFileHip

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLES = sorted(glob.glob(os.path.join(HERE, "golden", "ref_samples", "*.gvrs")))


def answer(image):
    f = GvrsFileHip(image)
    return R.inspect(image, R.facts_of(f)), f


def test_the_reference_samples_pass():
    assert len(SAMPLES) == 15
    for path in SAMPLES:
        image = open(path, "rb").read()
        a, f = answer(image)
        assert (a["failed"], a["complete"], a["stop"], a["bad_tiles"]) == (0, 1, R.END, []), path
        assert a["tile_dir_passed"] == int(bool(f.info["checksum_enabled"])), path
        walked = list(gvrs_walk.walk_records(image))
        assert a["n_records"] == len(walked) and a["termination_pos"] == len(image), path
        assert [(r[0], r[1], r[2]) for r in a["records"]] == [(w[0], w[1], w[2]) for w in walked], path
        assert a["n_by_type"][2] == sum(1 for w in walked if w[2] == 2) and a["n_by_type"][5] == 1
        assert all(r[4] == (1 if f.info["checksum_enabled"] else -1) for r in a["records"])


def test_sound_cases_pass():
    seg, chunk = K.plan()
    for name, image in K.sound_cases().items():
        a, f = answer(image)
        assert (a["failed"], a["complete"], a["stop"], a["bad_tiles"], a["reference"]) == (0, 1, R.END, [], {}), name
        assert a["tile_dir_passed"] == int(bool(f.info["checksum_enabled"])), name
        assert len(image) - a["termination_pos"] in (0, 8), name
        assert len(image) - f.info["content_pos"] >= 3 * seg or name in ("one tile", "updated", "free space directory"), name
    long_one = answer(K.sound_cases()["long both"])[0]
    assert sum(1 for r in long_one["records"] if r[1] > 2 * seg) == 3
    assert any(r[1] - 4 > K.WAVE_CHUNKS * chunk and (r[1] - 4) % chunk == chunk - 4 for r in answer(K.sound_cases()["metadata of whole chunks"])[0]["records"])
    a, f = answer(K.sound_cases()["starts on a seam"])
    assert sum(1 for r in a["records"] if (r[0] - f.info["content_pos"]) % seg == 0 and r[2] == 2) >= 3
    assert answer(K.sound_cases()["free space directory"])[0]["n_by_type"][3] == 1


# name -> (stop, complete, failed, bad tiles or their count or None, checksum failures or None)
WANT = {
    "flipped tile": (R.END, 1, 1, 1, 1),
    "tile and tile": (R.TWO_CHECKSUM_FAILURES, 0, 1, 2, 2),
    "tile and metadata": (R.TWO_CHECKSUM_FAILURES, 0, 1, 1, 2),
    "metadata and tile": (R.TWO_CHECKSUM_FAILURES, 0, 1, 1, 2),
    "three in a row": (R.TWO_CHECKSUM_FAILURES, 0, 1, 2, 2),
    "a good record between": (R.END, 1, 1, 2, 2),
    "tile directory fails": (R.END, 1, 1, 0, 1),
    "tile directory body": (R.END, 1, 1, 0, 1),
    "free head fails": (R.END, 1, 1, 0, 1),
    "free checksum word": (R.END, 1, 1, 0, 1),
    "tile index -1": (R.BAD_TILE_INDEX, 0, 1, 0, 0),
    "tile index = count": (R.BAD_TILE_INDEX, 0, 1, 0, 0),
    "tile too large": (R.TILE_TOO_LARGE, 0, 1, [20], 0),
    "type 7": (R.BAD_RECORD_TYPE, 0, 1, 0, 0),
    "type 255": (R.BAD_RECORD_TYPE, 0, 1, 0, 0),
    "zero size": (R.END, 1, 0, 0, 0),
    "size -8": (R.BAD_RECORD_SIZE, 0, 1, 0, 0),
    "size 8": (R.BAD_RECORD_SIZE, 0, 1, 0, 0),
    "size 20": (R.BAD_RECORD_SIZE, 0, 1, 0, 0),
    "size past the image": (R.TRUNCATED, 0, 1, 0, 0),
    "large tile past the image": (R.TILE_TOO_LARGE, 0, 1, 1, 0),
    "size into the next record": (None, None, 1, None, None),
    "size over the next record": (R.END, 1, 1, 0, 1),
    "stop in front of a double": (R.BAD_RECORD_TYPE, 0, 1, 0, 0),
    "double in front of a stop": (R.TWO_CHECKSUM_FAILURES, 0, 1, 2, 2),
    "first record": (R.BAD_RECORD_TYPE, 0, 1, 0, 0),
    "old copy fails": (R.END, 1, 1, [3], 1),
    "rejoins": (R.TWO_CHECKSUM_FAILURES, 0, 1, 0, 2),
    "rejoins without checksums": (R.END, 1, 0, 0, 0),
    "no checksums, past the image": (R.TRUNCATED, 0, 1, 0, 0),
    "no checksums, flipped": (R.END, 1, 0, 0, 0),
}


def test_damaged_cases_answer_as_stated():
    cases = K.damaged_cases()
    assert sorted(cases) == sorted(WANT)
    for name, image in cases.items():
        a, f = answer(image)
        stop, complete, failed, bad, fails = WANT[name]
        assert a["failed"] == failed, name
        if stop is not None:
            assert (a["stop"], a["complete"]) == (stop, complete), name
        if bad is not None:
            assert (a["bad_tiles"] == bad) if isinstance(bad, list) else (a["n_bad_tiles"] == bad), name
        if fails is not None:
            assert a["n_checksum_failures"] == fails, name
        assert a["bad_tile_index"] == int(a["stop"] == R.BAD_TILE_INDEX) and a["invalid_record_size"] == int(a["stop"] == R.TILE_TOO_LARGE)
        if a["stop"] != R.END:                                     # the stop record is the list's last, at the termination position
            assert a["records"][-1][0] == a["termination_pos"] and a["complete"] == 0, name
            assert a["records"][-1][4] == (0 if a["stop"] == R.TWO_CHECKSUM_FAILURES else -1), name


def test_the_deviations_are_pinned():
    cases = K.damaged_cases()
    for name in ("type 7", "type 255", "first record", "stop in front of a double"):
        a, _ = answer(cases[name])
        assert a["reference"] == {"termination_pos": 16} and a["termination_pos"] == a["records"][-1][0] > 16, name
    for name in ("size -8", "size 8", "size 20"):
        assert answer(cases[name])[0]["reference"] == {"undefined": True}, name
    a, _ = answer(cases["no checksums, past the image"])
    assert a["reference"]["complete"] == 1 and a["complete"] == 0 and a["reference"]["termination_pos"] > len(cases[name])
    assert answer(cases["size past the image"])[0]["reference"] == {}          # (with checksums the reference fails too: EOFException)
    a, _ = answer(cases["zero size"])                                           # a clean end in mid-file: fewer records, nothing failed
    assert a["n_records"] < answer(K.sound_cases()["shuffled"])[0]["n_records"] and a["termination_pos"] < len(cases["zero size"]) - 100


def test_the_two_failures_stop_at_the_second():
    cases = K.damaged_cases()
    for name in ("tile and tile", "three in a row", "double in front of a stop"):
        a, _ = answer(cases[name])
        assert [r[4] for r in a["records"][-2:]] == [0, 0] and all(r[4] == 1 for r in a["records"][:-2]), name
    a, _ = answer(cases["a good record between"])
    fails = [k for k, r in enumerate(a["records"]) if r[4] == 0]
    assert len(fails) == 2 and fails[1] == fails[0] + 2


@pytest.mark.parametrize("cut", [0, 1, 11, 12, 13, 20])
def test_the_last_bytes(cut):
    """fewer than 13 bytes behind a record end the walk cleanly; a record cut short is TRUNCATED"""
    image = K.sound_cases()["compact"]
    f = GvrsFileHip(image)
    recs = R.inspect(image, R.facts_of(f))["records"]
    end = recs[-2][0] + recs[-2][1]                                # (the tile directory starts here)
    a = R.inspect(image[:end + cut], R.facts_of(f))
    assert (a["stop"], a["complete"]) == ((R.END, 1) if cut <= 12 else (R.TRUNCATED, 0))
    assert a["termination_pos"] == end and a["n_records"] == len(recs) - (1 if cut <= 12 else 0)
