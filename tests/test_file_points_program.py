"""tests/csrc/file_points_test.cpp, the stand-alone program around gvrs_file_points.h, built plain and under the address and
undefined-behaviour sanitizers and run on the CPU over the cases of file_points_cases.py; its lines are compared with those of the
numpy restatement file_points_ref.py.  Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import pytest

import file_points_cases as K
import file_points_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GRIDS = K.SAMPLE_GRIDS + K.EXTRA_GRIDS


def build(tmp_path_factory, sanitized):
    out = str(tmp_path_factory.mktemp("file_points") / ("file_points_test" + ("_san" if sanitized else "")))
    # (as test_file_inspect_program.py builds its program; gvrs_interp_common.h, which the header includes, carries hipcc's unroll
    # pragmas and is built without contraction wherever it is built)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off"]
    cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitized else []
    r = subprocess.run(cmd + ["-o", out, os.path.join(HERE, "csrc", "file_points_test.cpp")], capture_output=True, text=True)
    return out if r.returncode == 0 else None, r.stderr


def tail(grid, touched):
    _, _, slots = R.slots(grid, touched.tolist())
    assert slots == list(range(touched.size))                    # the restatement's own rule: a tile's slot is its rank
    return "; tiles" + "".join(" %d" % t for t in touched) + "; slots ok"


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """(the path of the cases' file, the lines the program must print for it)"""
    lines, want = [], []
    for grid in GRIDS:
        rows, cols = K.cell_points(grid)
        lines.append("cells %d %d %d %d %d " % (grid + (rows.size,)) + " ".join("%d %d" % rc for rc in zip(rows.tolist(), cols.tolist())))
        inside, tile, at = R.cell_tiles(grid, rows, cols)
        want.append("cells:" + "".join(" %d:%d" % (t, a) if i else " x" for i, t, a in zip(inside.tolist(), tile.tolist(), at.tolist()))
                    + tail(grid, R.cells_touched(grid, rows, cols)))
        drows, dcols = K.window_points(grid)
        for wrap in (0, 1, 2):
            for k in range(len(K.FRINGES)):
                rf, cf = K.fringe_of(grid, k)
                spec = R.spec_of(grid, wrap, rf, cf)
                lines.append("windows %d %d %d %d %d %s %s %s %s %d " % (grid + (wrap,) + tuple(x.hex() for x in spec.row_fringe + spec.col_fringe)
                                                                       + (drows.size,))
                             + " ".join("%s %s" % (r.hex(), c.hex()) for r, c in zip(drows.tolist(), dcols.tolist())))
                per_point = R.window_tiles(grid, spec, drows, dcols)
                want.append("windows:" + "".join(" " + ",".join(str(t) for t in p) if p else " x" for p in per_point)
                            + tail(grid, R.windows_touched(grid, spec, drows, dcols)))
    path = str(tmp_path_factory.mktemp("file_points_cases") / "cases.txt")
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
        assert line == w, k


def test_points_path_alone(tmp_path_factory, cases):
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


def test_points_path_alone_under_the_sanitizers(tmp_path_factory, cases):
    if not sanitizer_runtime(tmp_path_factory):
        pytest.skip("the sanitizer runtime is not installed: the plain program runs in test_points_path_alone")
    out, err = build(tmp_path_factory, True)
    assert out, err[-4000:]                                        # (with the runtime there, a failing build is a failure)
    run(out, cases)
