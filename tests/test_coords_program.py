"""tests/csrc/coords_test.cpp, the stand-alone program around gvrs_coords.h, built plain and under the address and
undefined-behaviour sanitizers and run on the CPU over the cases of coords_cases.py, doubles passed as hexadecimal floats; its
lines are compared, value by value and bit by bit, with those of the Python restatement coords_ref.py.  Nothing loaded into Python
runs under a sanitizer."""
import math
import os
import subprocess

import pytest

import coords_cases as K
import coords_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def build(tmp_path_factory, sanitized):
    out = str(tmp_path_factory.mktemp("coords") / ("coords_test" + ("_san" if sanitized else "")))
    # (as test_file_points_program.py builds its program)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off"]
    cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitized else []
    r = subprocess.run(cmd + ["-o", out, os.path.join(HERE, "csrc", "coords_test.cpp")], capture_output=True, text=True)
    return out if r.returncode == 0 else None, r.stderr


def hx(v):
    v = float(v)
    return "nan" if v != v else ("inf" if v == math.inf else "-inf" if v == -math.inf else v.hex())


def key(v):
    """what a printed double is compared by: its bits, or "nan" """
    v = float(v)
    return "nan" if v != v else R.bits(v)


def parse(token):
    return "nan" if token == "nan" else R.bits(float(token) if "inf" in token else float.fromhex(token))


COS_ARGS = [0.0, -0.0, 1e-9, 2.0 ** -27, 0.29, 0.3, 0.31, 0.78, 0.7853981633974483, 0.79, 1.0, -1.0, 1.5, 1.5707963, 1.5707963267948966,
            -1.5707963267948966, 1.6, 2.3, -2.3, 2.4, 1e300, math.inf, math.nan] + [R.to_radians(v) for v in K.COS_TELLING + [90.0, -90.0, 90.0001, -90.0001]]
ANGLES = [0.0, -0.0, 180.0, -180.0, 360.0, -360.0, 540.0, -540.0, 190.0, -190.0, 10.0, -10.0, 179.999999, -181.0, 725.0, 1e300, -1e300, math.inf,
          -math.inf, math.nan]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """(the path of the cases' file, per line the values the program must print: keys of doubles and ints)"""
    lines, want = [], []
    lines.append("cos %d " % len(COS_ARGS) + " ".join(hx(v) for v in COS_ARGS))
    want.append([[key(R.strict_cos(v))] for v in COS_ARGS])
    lines.append("angle %d " % len(ANGLES) + " ".join(hx(v) for v in ANGLES))
    want.append([[key(R.to180(v)), key(R.to360(v))] for v in ANGLES])
    for name in K.GRIDS:
        info, co = K.info_of(name), K.coords_of(name)
        lines.append("file %d %d %d " % (info["grid"][0], info["grid"][1], info["coordinate_system"])
                     + " ".join(hx(info[k]) for k in ("x0", "y0", "x1", "y1", "cell_size_x", "cell_size_y")) + " "
                     + " ".join(hx(v) for v in list(info["m2r"]) + list(info["r2m"])))
        want.append([[co.wrap]] + [[key(v)] for v in (co.row_fringe + co.col_fringe + (co.du, co.dv))])
        x, y = K.file_points(name)
        rows, cols = K.grid_points(name)
        for kind, (a, b) in ((R.GEO_TO_GRID, (x, y)), (R.MODEL_TO_GRID, (x, y)), (R.GRID_TO_GEO, (rows, cols)), (R.GRID_TO_MODEL, (rows, cols))):
            lines.append("map %d %d " % (kind, a.size) + " ".join("%s %s" % (hx(p), hx(q)) for p, q in zip(a.tolist(), b.tolist())))
            per = []
            for p, q in zip(a.tolist(), b.tolist()):
                m = co.map_point(kind, p, q)
                per.append([key(m[0]), key(m[1])] + ([m[2], m[3], key(m[4]), m[5]] if kind < R.GRID_TO_GEO else []))
            want.append(per)
        for kind, (a, b) in ((R.COORDS_GRID, (rows, cols)), (R.COORDS_FILE, (x, y))):
            lines.append("query %d %d " % (kind, a.size) + " ".join("%s %s" % (hx(p), hx(q)) for p, q in zip(a.tolist(), b.tolist())))
            per = []
            for p, q in zip(a.tolist(), b.tolist()):
                st, row, col, cs = co.query(kind, p, q)
                per.append([st, key(row), key(col), key(cs)])
            want.append(per)
    path = str(tmp_path_factory.mktemp("coords_cases") / "cases.txt")
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
        head, tokens = line.split(":")[0], line.split(":", 1)[1].split()
        if head == "file":
            tokens = [tokens[0]] + tokens[1:]
            got = [[int(tokens[0])]] + [[parse(t)] for t in tokens[1:]]
        else:
            got = []
            for t in tokens:
                parts = t.split(",")
                if head == "map" and len(parts) == 6:
                    got.append([parse(parts[0]), parse(parts[1]), int(parts[2]), int(parts[3]), parse(parts[4]), int(parts[5])])
                elif head == "query":
                    got.append([int(parts[0])] + [parse(p) for p in parts[1:]])
                else:
                    got.append([parse(p) for p in parts])
        assert len(got) == len(w), (k, head)
        for i, (g, x) in enumerate(zip(got, w)):
            assert g == x, (k, head, i)


def test_coords_alone(tmp_path_factory, cases):
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


def test_coords_alone_under_the_sanitizers(tmp_path_factory, cases):
    if not sanitizer_runtime(tmp_path_factory):
        pytest.skip("the sanitizer runtime is not installed: the plain program runs in test_coords_alone")
    out, err = build(tmp_path_factory, True)
    assert out, err[-4000:]                                        # (with the runtime there, a failing build is a failure)
    run(out, cases)
