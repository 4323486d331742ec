"""tests/csrc/file_update_test.cpp, the stand-alone program around gvrs_file_update.h, built plain and under the address and
undefined-behaviour sanitizers and run on the CPU over the reference's sample files, over images with free space
(tests/file_update_cases.py) and over all their truncations.  Nothing loaded into Python runs under a sanitizer."""
import glob
import os
import subprocess

import pytest

import file_update_cases as U

HERE = os.path.dirname(os.path.abspath(__file__))


def build(tmp_path_factory, sanitized):
    out = str(tmp_path_factory.mktemp("file_update") / ("file_update_test" + ("_san" if sanitized else "")))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
    cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitized else []
    r = subprocess.run(cmd + ["-o", out, os.path.join(HERE, "csrc", "file_update_test.cpp")], capture_output=True, text=True)
    return out if r.returncode == 0 else None, r.stderr


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    d = tmp_path_factory.mktemp("file_update_images")
    paths = sorted(glob.glob(os.path.join(HERE, "golden", "ref_samples", "*.gvrs")))
    assert len(paths) == 15
    made = {"base": U.make_file(U.BASE), "base_nocrc": U.make_file(U.BASE, checksums=False), "roomy": U.make_file(U.BASE, free_dir_slack=1),
            "extended": U.make_file(U.BASE, extended=True), "small_rect": U.make_file([("t", 44, 40), ("f", 64), ("t", 55, 40)], dir_rect=(4, 4, 2, 2))}
    image, records, tiles, *_ = U.scenario("replace frees first")
    made["updated"] = U.model(image, records, tiles)[0]
    for name, data in made.items():
        p = str(d / (name + ".gvrs"))
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
    return paths


def run(exe, images):
    r = subprocess.run([exe] + images, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-3000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "done" and len(lines) == len(images) + 1
    assert all(line.endswith(" 0 truncations opened") for line in lines[:-1])      # a truncated file is never taken for a whole one


def test_update_path_alone(tmp_path_factory, images):
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


def test_update_path_alone_under_the_sanitizers(tmp_path_factory, images):
    if not sanitizer_runtime(tmp_path_factory):
        pytest.skip("the sanitizer runtime is not installed: the plain program runs in test_update_path_alone")
    out, err = build(tmp_path_factory, True)
    assert out, err[-4000:]                                        # (with the runtime there, a failing build is a failure)
    run(out, images)
