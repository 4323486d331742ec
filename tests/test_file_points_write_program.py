"""tests/csrc/file_points_write_test.cpp, the stand-alone program around gvrs_file_points_store.h (the cell rule that the block
write and the writes at scattered points share), built plain and under the address and undefined-behaviour sanitizers and run on
the CPU over the values of file_points_write_cases.py; its lines are compared, value for value, with the table of the numpy model
block_write_ref.py.  Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

import block_write_ref as BW
import file_points_write_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = {"int": 0, "short": 1, "float": 2, "icf": 3}


def build(tmp_path_factory, sanitized):
    out = str(tmp_path_factory.mktemp("file_points_write") / ("file_points_write_test" + ("_san" if sanitized else "")))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off"]
    cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitized else []
    r = subprocess.run(cmd + ["-o", out, os.path.join(HERE, "csrc", "file_points_write_test.cpp")], capture_output=True, text=True)
    return out if r.returncode == 0 else None, r.stderr


def word(x, dtype):
    return int(K.bits(np.array([x]), dtype)[0])


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """(the path of the cases' file, the lines the program must print for it)"""
    lines, want = [], []
    for el, fill, values in K.CASES:
        kind = BW.kind_of(el)
        dt = BW.tile_dtype(el) if kind != "icf" else np.float32          # the type the VALUES travel in
        lo, hi = BW.default_range(el)
        if kind in ("int", "short"):
            head = [word(fill, dt), 0, word(lo, np.int32), word(hi, np.int32), word(1.0, np.float32), word(0.0, np.float32)]
        elif kind == "float":
            head = [word(fill, np.float32), word(fill, np.float32), word(lo, np.float32), word(hi, np.float32), word(1.0, np.float32), 0]
        else:
            head = [word(el[3], np.int32), word(el[4], np.float32), word(lo, np.float32), word(hi, np.float32), word(el[1], np.float32),
                    word(el[2], np.float32)]
        vb = K.bits(values, dt)
        lines.append("%d " % KINDS[kind] + " ".join("%x" % h for h in head) + " %d " % vb.size + " ".join("%x" % v for v in vb))
        stored, cell, valid = K.expected(el, fill, values)
        want.append("".join(" %d:%x:%d" % (s, c, v) for s, c, v in zip(stored.tolist(), cell.tolist(), valid.tolist())))
    path = str(tmp_path_factory.mktemp("file_points_write_cases") / "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path, want


def run(exe, cases):
    path, want = cases
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-3000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "done" and len(lines) == len(want) + 1
    for k, (line, w) in enumerate(zip(lines, want)):
        assert line == w, (k, K.CASES[k][0], line, w)


def test_every_edge_is_in_the_table():
    """the table itself: each kind refuses something, stores its fill, and stores a cell that is data"""
    for el, fill, values in K.CASES:
        stored, _, valid = K.expected(el, fill, values)
        assert stored.any() and valid.any() and (stored & ~valid).any(), el
    assert all(any((~K.expected(el, f, v)[0]).any() for el, f, v in K.CASES if BW.kind_of(el) == k) for k in ("int", "short", "icf"))


def test_store_rule_alone(tmp_path_factory, cases):
    out, err = build(tmp_path_factory, False)
    assert out, err[-4000:]
    run(out, cases)


def sanitizer_runtime(tmp_path_factory):
    """can this machine link and run a program under the two sanitizers at all?"""
    d = tmp_path_factory.mktemp("san_probe")
    src, exe = str(d / "probe.cpp"), str(d / "probe")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-o", exe, src], capture_output=True, text=True)
    return r.returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0


def test_store_rule_alone_under_the_sanitizers(tmp_path_factory, cases):
    if not sanitizer_runtime(tmp_path_factory):
        pytest.skip("the sanitizer runtime is not installed: the plain program runs in test_store_rule_alone")
    out, err = build(tmp_path_factory, True)
    assert out, err[-4000:]                                        # (with the runtime there, a failing build is a failure)
    run(out, cases)
