"""gridfour_amd/csrc/gvrs_lsop_container.h, the host's half of the LSOP12 and LSOP08 encoders, on its own:
tests/csrc/lsop_container_test.cpp is a stand-alone program built with the address and undefined-behaviour sanitizers.  It is given
what the device encoder leaves for the host -- residual streams, coefficient records, the device's packings and statuses, all taken
from the references (lsop_container_cases.py) -- and must print the references' blob, offsets, container types and statuses byte
for byte: oracle.lsop12_encode and lsop08_ref.encode."""
import os
import struct
import subprocess

import numpy as np
import pytest

import lsop_container_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
OK, DECLINED, ERR_CAPACITY = 0, 1, -3


@pytest.fixture(scope="module")
def exe():
    path = os.path.join(HERE, "csrc", "lsop_container_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", path, os.path.join(HERE, "csrc", "lsop_container_test.cpp"), "-lz"])
    return path


def run(exe, tmp_path, b, blob_cap):
    """the program on batch b with a blob of blob_cap bytes: (return value, blob, offsets, types, statuses)"""
    case = struct.pack("<6IQ", b.family, K.CODEC_INDEX, b.nr, b.nc, b.flags, len(b.tiles), blob_cap)
    for t in b.tiles:
        assert t.residuals.size == b.n_res and t.residuals.dtype == np.int32 and t.coefs.dtype == np.uint32
        case += struct.pack("<iI", t.status, len(t.device)) + t.device + t.coefs.tobytes() + t.residuals.tobytes()
    path = os.path.join(str(tmp_path), b.name + ".case")
    with open(path, "wb") as f:
        f.write(case)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    out = dict(line.split(" ", 1) for line in r.stdout.splitlines())
    ints = lambda key: [int(x) for x in out[key].split()]
    return int(out["rc"]), bytes.fromhex(out["blob"].strip()), ints("offsets"), ints("types"), ints("status")


def outcomes(name):
    return [(t.status, t.want_type, None if t.want is None else len(t.want)) for t in K.batch(name).tiles]


def test_the_references_give_every_outcome():
    """before the program is looked at: each way the choice can go occurs among the cases (sizes as the references give them)"""
    assert outcomes("lsop12_48") == [(OK, 2, 1211), (DECLINED, 0, None), (OK, 1, 4699)]       # type 2, declined between two good ones, type 1
    assert outcomes("lsop12_48_checksum") == [(OK, 2, 1215), (DECLINED, 0, None), (OK, 1, 4703)]
    assert outcomes("lsop12_48_no_deflate") == [(OK, 2, 1211), (DECLINED, 0, None), (OK, 2, 7119)]
    assert outcomes("lsop12_6") == [(OK, 2, 96)]
    assert outcomes("lsop08_6") == [(OK, 0, 91)] and len(K.batch("lsop08_6").tiles[0].device) == 91
    assert outcomes("lsop08_7x9") == [(OK, 1, 119), (DECLINED, 0, None), (OK, 1, 128)]
    assert outcomes("lsop08_4") == [(OK, 0, 66)]
    import lsop08_ref as R
    sizes = lambda b, i: [len(R.encode(K.CODEC_INDEX, b.nr, b.nc, b.values[i], force_type=ft)[0]) for ft in (0, 1)]
    assert sizes(K.batch("lsop08_6"), 0) == [91, 99] and sizes(K.batch("lsop08_4"), 0) == [66, 78]
    assert sizes(K.batch("lsop08_7x9"), 0) == [121, 119]
    assert sizes(K.batch("lsop08_7x9"), 2) == [128, 128]                                    # the tie: type 1
    for name in ("lsop12_48", "lsop12_48_checksum"):                                        # LSOP12 keeps type 2 only where it is no longer
        t = K.batch(name).tiles[2]
        assert len(t.want) < len(t.device)


@pytest.mark.parametrize("name", list(K.BATCHES))
def test_container_choice_and_blob(exe, tmp_path, name):
    b = K.batch(name)
    want_blob, want_offsets, want_types, want_status = b.want_blob()
    rc, blob, offsets, types, status = run(exe, tmp_path, b, len(want_blob) + 5)
    assert rc == OK and (offsets, types, status) == (want_offsets, want_types, want_status)
    assert blob == want_blob + b"\xee" * 5


@pytest.mark.parametrize("name", ["lsop12_48", "lsop08_7x9"])
def test_blob_one_byte_short(exe, tmp_path, name):
    b = K.batch(name)
    want_blob, want_offsets, want_types, want_status = b.want_blob()
    rc, blob, offsets, types, status = run(exe, tmp_path, b, len(want_blob) - 1)
    assert rc == ERR_CAPACITY and (offsets, types, status) == (want_offsets, want_types, want_status)
    assert blob == b"\xee" * (len(want_blob) - 1)
