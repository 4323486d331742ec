"""CodecCanonHuffmanHip's analysis in the C++ host mirror (gridfour_amd/host/gvrs_hip_codec.hpp): the no-device path on the
CPU, and on the GPU the same sums, escape table and report as the Python class."""
import io
import os
import subprocess

import numpy as np
import pytest

import gridfour_amd
import oracle
from tilegen import make_tile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build(tmp_path):
    gridfour_amd.lib()                                        # makes sure libgvrs_hip.so exists
    exe = str(tmp_path / "canon_analyze_mirror_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "csrc", "canon_analyze_mirror_test.cpp"),
                           "-L" + os.path.join(ROOT, "gridfour_amd", "lib"), "-lgvrs_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "gridfour_amd", "lib"), "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_canon_analysis_fails_loudly_without_gpu(tmp_path):
    exe = _build(tmp_path)
    if gridfour_amd.lib().gf_device_count() > 0:
        pytest.skip("a GPU is present")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 10 and "no-device" in r.stdout, r.stdout


@pytest.mark.gpu
def test_cpp_canon_analysis_matches_python(tmp_path):
    exe = _build(tmp_path)
    nr, nc = 48, 64
    tiles = [make_tile(k, nr, nc, seed=s) for s, k in enumerate(["smooth", "noise16", "uniform", "sparse_big", "steps"])]
    packs = [oracle.codec_canon_encode(0, nr, nc, t)[0] for t in tiles]
    packs.append(packs[0][:1] + bytes([5]) + packs[0][2:])            # "All Predictors" twice
    packs.append(packs[1][:1] + bytes([9]) + packs[1][2:])            # throws after the escape table
    packs.append(packs[3][:20])                                       # truncated
    path = tmp_path / "packs.txt"
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (nr, nc, len(packs)))
        for p in packs:
            f.write("%d %s\n" % (len(p), " ".join("%02x" % b for b in p)))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    codec = gridfour_amd.CodecCanonHuffmanHip()
    st = codec.analyze_batch(nr, nc, packs)
    got, esc = codec.analysis_data(), codec.escape_counts()
    for tag in ("single", "batch"):
        rows = [line.split()[2:] for line in lines if line.startswith(tag + " ") and line.split()[1].isdigit()]
        assert len(rows) == 6
        for k, row in enumerate(rows):
            ints = [int(x) for i, x in enumerate(row) if i != 7]
            assert ints == [int(got[k][f]) for f in ("n_tiles", "n_bytes", "n_symbols", "n_bits_overhead", "n_text_counted",
                                                     "sum_length", "sum_observed", "sum_escape_bits")], (tag, k)
            assert float(row[7]) == pytest.approx(float(got[k]["sum_entropy"]), rel=1e-15)
        assert [int(x) for x in next(line for line in lines if line.startswith(tag + " escapes")).split()[2:]] == list(map(int, esc))
        status = [int(x) for x in next(line for line in lines if line.startswith(tag + " status")).split()[2:]]
        assert [s != 0 for s in status] == [s != 0 for s in st]
    assert int(got[5]["n_tiles"]) == 5 + 2 and sum(st != 0) == 2                  # (the byte-5 copy counts twice)
    out = io.StringIO()
    codec.reportAnalysisData(out, len(packs))
    cleared = "GVRS Canonical Huffman                          Compressed Output    |       Predictor Residuals\n   Tiles Compressed:  0\n"
    assert r.stdout.split("batch status")[1].split("\n", 1)[1] == out.getvalue() + cleared
