"""tests/csrc/file_inspect_test.cpp, the stand-alone program around gvrs_file_inspect.h, built plain and under the address and
undefined-behaviour sanitizers and run on the CPU over the reference's sample files, over the images of tests/inspect_cases.py
and over all their truncations; its verdicts are compared with the restatement's.  Nothing loaded into Python runs under a
sanitizer."""
import glob
import os
import subprocess

import pytest

import gvrs_inspect_ref as R
import inspect_cases as K
from gridfour_amd import GvrsFileHip

HERE = os.path.dirname(os.path.abspath(__file__))


def build(tmp_path_factory, sanitized):
    out = str(tmp_path_factory.mktemp("file_inspect") / ("file_inspect_test" + ("_san" if sanitized else "")))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
    cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitized else []
    r = subprocess.run(cmd + ["-o", out, os.path.join(HERE, "csrc", "file_inspect_test.cpp")], capture_output=True, text=True)
    return out if r.returncode == 0 else None, r.stderr


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    """[(path, the line the program must print for it, without the path)]"""
    d = tmp_path_factory.mktemp("file_inspect_images")
    paths = sorted(glob.glob(os.path.join(HERE, "golden", "ref_samples", "*.gvrs")))
    assert len(paths) == 15
    for k, (name, data) in enumerate(K.all_cases().items()):
        p = str(d / ("case%02d.gvrs" % k))
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
    out = []
    for p in paths:
        data = open(p, "rb").read()
        f = GvrsFileHip(data)
        a = R.inspect(data, R.facts_of(f))
        out.append((p, "%d bytes, %d records, stop %d, failed %d, complete %d, dir %d, end %d, %d bad, %d failures, %d truncations walked" % (
            len(data), a["n_records"], a["stop"], a["failed"], a["complete"], a["tile_dir_passed"], a["termination_pos"], a["n_bad_tiles"],
            a["n_checksum_failures"], len(data) - f.info["content_pos"])))
    return out


def run(exe, images):
    r = subprocess.run([exe] + [p for p, _ in images], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-3000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "done" and len(lines) == len(images) + 1
    for line, (p, want) in zip(lines, images):
        assert line == p + ": " + want


def test_inspect_path_alone(tmp_path_factory, images):
    out, err = build(tmp_path_factory, False)
    assert out, err[-4000:]
    run(out, images)


def sanitizer_runtime(tmp_path_factory):
    """can this machine link and run a program under the two sanitizers at all?"""
    d = tmp_path_factory.mktemp("san_probe")
    src, exe = str(d / "probe.cpp"), str(d / "probe")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-o", exe, src], capture_output=True, text=True)
    return r.returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0


def test_inspect_path_alone_under_the_sanitizers(tmp_path_factory, images):
    if not sanitizer_runtime(tmp_path_factory):
        pytest.skip("the sanitizer runtime is not installed: the plain program runs in test_inspect_path_alone")
    out, err = build(tmp_path_factory, True)
    assert out, err[-4000:]                                        # (with the runtime there, a failing build is a failure)
    run(out, images)
