"""gridfour_amd/csrc/gvrs_stage.h, the staging of one host-form call, on its own: tests/csrc/stage_test.cpp is a stand-alone
program built with the address and undefined-behaviour sanitizers.  Its device is a malloc of exactly the laid-out total and its
copier is memcpy.  Parts start at multiples of 16 and do not overlap, inputs arrive intact with their slack inside the total,
outputs and in-out parts come home, a fetch copies its prefix only, absent and empty parts read as the header says, a zeroed part
is zero in a dirty buffer, a buffer in use refuses a second stage and is given back on every way out, and one declaration more
than the table holds is refused."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_stage_header_under_sanitizers():
    exe = os.path.join(HERE, "csrc", "stage_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "csrc", "stage_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and not r.stderr, r.stdout + r.stderr
