"""gridfour_amd/csrc/gvrs_carve.h, the layout helper of the C ABI's multi-part buffers, on its own: tests/csrc/carve_test.cpp is a
stand-alone program built with the address and undefined-behaviour sanitizers.  Offsets are multiples of 16, parts do not overlap,
the total is the sum of the rounded parts, zero-byte parts are allowed, the per-element form equals the loop it replaced, and
every part written full stays inside a malloc of exactly the total."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_carve_header_under_sanitizers():
    exe = os.path.join(HERE, "csrc", "carve_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "csrc", "carve_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and not r.stderr, r.stdout + r.stderr
