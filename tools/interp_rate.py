"""What B-spline interpolation over a device-resident block costs: the ETOPO1-shaped float block, 10,800 x 21,600 cells, sampled on a
lattice of the same size offset by half a cell (233 million points).
    python tools/interp_rate.py [--out profiles/interp_rate.json] [--shrink K]
HIP events on the context's stream, 20 timings per case taken in turn in one process; medians, min and max.  Before the timings the
value outputs of the lattice form, of the points form and of the CPU harness are compared bit for bit.
  lattice_value / lattice_first_normal   gf_block_interp_lattice_dev (k_interp_lattice): z alone; z, zx, zy and the unit normal
  lattice_rows_value                     the same lattice with a column spacing per lattice row: k_interp_points generating the coordinates
  points_value / points_first_normal     gf_block_interp_points_dev on the lattice's coordinates, in order
  points_shuffled_value                  ... on the same coordinates in a random order
  copy_d2d                               a device-to-device copy of the value output's bytes: the memory yardstick
  host_value / host_first_normal         what a caller had before: the block copied to the host, evaluated by the stand-alone C++
                                         harness (tests/csrc/interp_harness.cpp, g++ -O2 -ffp-contract=off) on 16 threads, the results
                                         copied back; wall clock, 3 timings
No threshold is set: the numbers are written as they come out.  --shrink K divides both sides of the block by K (a quick look)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gridfour_amd  # noqa: E402
from gridfour_amd import DeviceBuffer, lib  # noqa: E402
from gridfour_amd import build as hipbuild  # noqa: E402
from gridfour_amd._lib import check  # noqa: E402
import interp_cases as K  # noqa: E402
import interp_ref as R  # noqa: E402

REPS, HOST_REPS, HOST_THREADS = 20, 3, 16


def _hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("libamdhip64 not loadable")


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _stats(v, reps):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": reps}


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    shrink = int(argv[argv.index("--shrink") + 1]) if "--shrink" in argv else 1
    n_rows, n_cols = 10800 // shrink, 21600 // shrink
    n = n_rows * n_cols
    L, hip = lib(), _hip()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    ih = K.build_harness()
    ctx = gridfour_amd.GvrsHipContext(0)
    timer = gridfour_amd.GpuTimer(ctx)
    stream = C.c_void_p(ctx.stream)
    rng = np.random.default_rng(20)
    block = (rng.standard_normal((n_rows, n_cols), dtype=np.float32) * np.float32(1000.0)).astype(np.float32)
    lattice = (0.5, 0.5, 1.0, 1.0, n_rows, n_cols)
    rows, cols = R.lattice_coords(*lattice)
    perm = rng.permutation(n)
    specs = {t: gridfour_amd.interp_spec(n_rows, n_cols, target=t, row_spacing=1855.0, col_spacing=1391.0) for t in (0, 1)}
    model = {t: R.Spec(n_rows, n_cols, target=t, row_spacing=1855.0, col_spacing=1391.0) for t in (0, 1)}

    print("inputs ready; uploading", file=sys.stderr, flush=True)
    d_block = DeviceBuffer(ctx, block.nbytes + 16).upload(block)
    d_rows, d_cols = DeviceBuffer(ctx, n * 8).upload(rows), DeviceBuffer(ctx, n * 8).upload(cols)
    d_rows_s, d_cols_s = DeviceBuffer(ctx, n * 8).upload(rows[perm]), DeviceBuffer(ctx, n * 8).upload(cols[perm])
    d_cs_rows = DeviceBuffer(ctx, n_rows * 8).upload(np.full(n_rows, 1391.0))
    d = {k: DeviceBuffer(ctx, n * (24 if k == "normal" else 8)) for k in ("z", "zx", "zy", "normal", "z2")}
    value, first = {"z": d["z"].ptr}, {k: d[k].ptr for k in ("z", "zx", "zy", "normal")}

    def copy_d2d():
        assert hip.hipMemcpyAsync(d["z2"].ptr, d["z"].ptr, n * 8, 3, stream) == 0                  # hipMemcpyDeviceToDevice

    cases = {
        "lattice_value": lambda: ctx.interp_lattice_dev(specs[0], d_block.ptr, lattice, value),
        "lattice_first_normal": lambda: ctx.interp_lattice_dev(specs[1], d_block.ptr, lattice, first),
        "lattice_rows_value": lambda: ctx.interp_lattice_dev(specs[0], d_block.ptr, lattice, value, d_cs_rows.ptr),
        "points_value": lambda: ctx.interp_points_dev(specs[0], d_block.ptr, n, d_rows.ptr, d_cols.ptr, value),
        "points_first_normal": lambda: ctx.interp_points_dev(specs[1], d_block.ptr, n, d_rows.ptr, d_cols.ptr, first),
        "points_shuffled_value": lambda: ctx.interp_points_dev(specs[0], d_block.ptr, n, d_rows_s.ptr, d_cols_s.ptr, value),
        "copy_d2d": copy_d2d,
    }

    # the host route: block down, the harness on 16 threads, results up
    h_block = np.empty_like(block)
    h = {k: np.empty(n * (3 if k == "normal" else 1)) for k in ("z", "zx", "zy", "normal")}

    def host_route(t):
        names = ("z",) if t == 0 else ("z", "zx", "zy", "normal")
        check(L.gf_dev_download(ctx.handle, _p(h_block), d_block.ptr, block.nbytes), "gf_dev_download")
        g = K.geom_of(model[t])
        ih.ih_interp_points(_p(g), _p(h_block), n, _p(rows), _p(cols), None, _p(h["z"]), *[_p(h[k]) if t else None for k in ("zx", "zy")],
                            None, None, None, _p(h["normal"]) if t else None, None, HOST_THREADS)
        for k in names:
            check(L.gf_dev_upload(ctx.handle, d[k if k != "z" else "z2"].ptr, _p(h[k]), h[k].nbytes), "gf_dev_upload")

    # every case once outside the timings; the three routes to z must agree in every bit
    cases["lattice_value"]()
    ctx.synchronize()
    z_lattice = d["z"].download(np.float64, n)
    cases["points_value"]()
    ctx.synchronize()
    z_points = d["z"].download(np.float64, n)
    cases["points_shuffled_value"]()
    ctx.synchronize()
    z_shuffled = d["z"].download(np.float64, n)
    cases["lattice_rows_value"]()
    ctx.synchronize()
    z_rows = d["z"].download(np.float64, n)
    host_route(0)
    agree = {"lattice_vs_points": R.same_bits(z_lattice, z_points), "lattice_vs_lattice_rows": R.same_bits(z_lattice, z_rows),
             "shuffled_vs_points": R.same_bits(z_shuffled, z_points[perm]), "harness_vs_lattice": R.same_bits(h["z"], z_lattice)}
    del z_lattice, z_points, z_shuffled, z_rows
    for k in ("lattice_first_normal", "points_first_normal", "copy_d2d"):
        cases[k]()
    ctx.synchronize()

    print("outputs compared: %s; timing" % agree, file=sys.stderr, flush=True)
    ms = {k: [] for k in cases}
    for _ in range(REPS):
        for k, fn in cases.items():
            timer.start()
            fn()
            timer.stop()
            ms[k].append(timer.elapsed_ms())
    r = {k: _stats(v, REPS) for k, v in ms.items()}
    print("device cases timed; the host route", file=sys.stderr, flush=True)
    for t, name in ((0, "host_value"), (1, "host_first_normal")):
        wall = []
        for _ in range(HOST_REPS):
            t0 = time.perf_counter()
            host_route(t)
            wall.append((time.perf_counter() - t0) * 1e3)
        r[name] = _stats(wall, HOST_REPS)
    for k, v in r.items():
        v["Mpoints_per_s"] = round(n / 1e6 / (v["median_ms"] / 1e3), 1)
    r["copy_d2d"]["GBps"] = round(n * 8 / 1e9 / (r["copy_d2d"]["median_ms"] / 1e3), 1)
    out = {"workload": "etopo1 shape: a FLOAT block of %d x %d cells interpolated on a lattice of %d x %d points offset by half a cell" %
                       (n_rows, n_cols, n_rows, n_cols),
           "method": "HIP events, %d timings per case taken in turn in one process; host_*: wall clock, %d timings, %d threads" %
                     (REPS, HOST_REPS, HOST_THREADS),
           "csrc_digest": hipbuild.csrc_digest(), "points": n, "block_bytes": int(block.nbytes), "value_output_bytes": n * 8,
           "outputs_agree_bit_for_bit": agree, "cases": r}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
