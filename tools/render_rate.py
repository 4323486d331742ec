"""What rendering a device-resident block to ARGB costs: the ETOPO1-shaped float block, 10,800 x 21,600 cells, rendered with the
reference's ETOPO1.cpt on a lattice of the same size offset by half a cell (233 million pixels), beside the interpolation kernel it
is measured against.
    python tools/render_rate.py [--out profiles/render_rate.json] [--shrink K]
HIP events on the context's stream, 20 timings per case taken in turn in one process; medians, min and max.  Before the timings the
fused kernel's words are compared with the unfused path's: gf_block_interp_lattice_dev's z and the fused kernel's own shade output
through the cells form.
  render_lattice_shaded       gf_block_render_lattice_dev (k_render_lattice) with ExtractData's light: first derivatives, shade, lookup;
                              one int32 per pixel stored
  render_lattice_value        the same without a light: the value alone, the lookup without shade
  render_lattice_rows_shaded  the same lattice with a column spacing per row: gf_block_render_points_dev (k_render_points)
  interp_first_z_zx_zy        THE YARDSTICK: gf_block_interp_lattice_dev, target FIRST, storing z, zx and zy only (24 bytes a pixel)
  render_cells                gf_block_render_cells_dev on the block's own float cells
  render_cells_shaded         ... with a shade array
  copy_d2d_cells              a device-to-device copy of the block's bytes: what render_cells reads and writes
No threshold is set here: the numbers are written as they come out.  --shrink K divides both sides of the block by K (a quick look)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gridfour_amd  # noqa: E402
from gridfour_amd import DeviceBuffer  # noqa: E402
from gridfour_amd import build as hipbuild  # noqa: E402
import render_cases as RC  # noqa: E402

REPS = 20


def _hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("libamdhip64 not loadable")


def _stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v)}


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    shrink = int(argv[argv.index("--shrink") + 1]) if "--shrink" in argv else 1
    n_rows, n_cols = 10800 // shrink, 21600 // shrink
    n = n_rows * n_cols
    hip = _hip()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    rng = np.random.default_rng(21)
    # smooth relief inside the palette's range with noise on top: neighbouring pixels mostly share a record, slopes of every sign
    y, x = np.linspace(0.0, 9.0, n_rows, dtype=np.float32)[:, None], np.linspace(0.0, 17.0, n_cols, dtype=np.float32)[None, :]
    block = (np.sin(y) * np.cos(x) * np.float32(6000.0) - np.float32(1500.0) + rng.standard_normal((n_rows, n_cols), dtype=np.float32) * np.float32(40.0)).astype(np.float32)
    lattice = (0.5, 0.5, 1.0, 1.0, n_rows, n_cols)
    palette_args = RC.cpt("ETOPO1.cpt")
    light = RC.LIGHTS["extract"]

    ctx = gridfour_amd.GvrsHipContext(0)
    timer = gridfour_amd.GpuTimer(ctx)
    stream = C.c_void_p(ctx.stream)
    pal = gridfour_amd.Palette(ctx, **palette_args)
    li = RC.lib_light(light)
    spec = gridfour_amd.interp_spec(n_rows, n_cols, target=1, row_spacing=1855.0, col_spacing=1391.0)
    print("inputs ready; uploading", file=sys.stderr, flush=True)
    d_block = DeviceBuffer(ctx, block.nbytes + 16).upload(block)
    d_cs_rows = DeviceBuffer(ctx, n_rows * 8).upload(np.full(n_rows, 1391.0))
    d = {k: DeviceBuffer(ctx, n * 8) for k in ("z", "zx", "zy", "shade")}
    d_argb, d_argb2 = DeviceBuffer(ctx, n * 4), DeviceBuffer(ctx, n * 4)
    first = {k: d[k].ptr for k in ("z", "zx", "zy")}

    def copy_d2d():
        assert hip.hipMemcpyAsync(d_argb2.ptr, d_block.ptr, n * 4, 3, stream) == 0                 # hipMemcpyDeviceToDevice

    cases = {
        "render_lattice_shaded": lambda: ctx.render_lattice_dev(spec, d_block.ptr, lattice, pal, {"argb": d_argb.ptr}, li),
        "render_lattice_value": lambda: ctx.render_lattice_dev(spec, d_block.ptr, lattice, pal, {"argb": d_argb.ptr}),
        "render_lattice_rows_shaded": lambda: ctx.render_points_dev(spec, d_block.ptr, pal, {"argb": d_argb.ptr}, lattice=lattice,
                                                                    d_col_spacing=d_cs_rows.ptr, light=li),
        "interp_first_z_zx_zy": lambda: ctx.interp_lattice_dev(spec, d_block.ptr, lattice, first),
        "render_cells": lambda: ctx.render_cells_dev(pal, "float", d_block.ptr, n, d_argb.ptr),
        "render_cells_shaded": lambda: ctx.render_cells_dev(pal, "float", d_block.ptr, n, d_argb.ptr, d["shade"].ptr),
        "copy_d2d_cells": copy_d2d,
    }

    # fused against unfused, every word: the fused kernel's argb and shade; the interpolator's z with that shade through the cells form
    ctx.render_lattice_dev(spec, d_block.ptr, lattice, pal, {"argb": d_argb.ptr, "shade": d["shade"].ptr}, li)
    cases["interp_first_z_zx_zy"]()
    ctx.render_cells_dev(pal, "z", d["z"].ptr, n, d_argb2.ptr, d["shade"].ptr)
    ctx.synchronize()
    fused, unfused = d_argb.download(np.uint32, n), d_argb2.download(np.uint32, n)
    cases["render_lattice_rows_shaded"]()
    ctx.synchronize()
    by_rows = d_argb.download(np.uint32, n)
    model = RC.M.Palette(**palette_args)
    agree = {"fused_vs_unfused": bool(np.array_equal(fused, unfused)), "lattice_vs_lattice_rows": bool(np.array_equal(fused, by_rows)),
             "null_colour_share": round(float((fused == model.argb_for_null).mean()), 4), "distinct_words": int(np.unique(fused).size)}
    del fused, unfused, by_rows
    for fn in cases.values():                                                                      # every case once outside the timings
        fn()
    ctx.synchronize()

    print("outputs compared: %s; timing" % agree, file=sys.stderr, flush=True)
    ms = {k: [] for k in cases}
    for _ in range(REPS):
        for k, fn in cases.items():
            timer.start()
            fn()
            timer.stop()
            ms[k].append(timer.elapsed_ms())
    r = {k: _stats(v) for k, v in ms.items()}
    for k, v in r.items():
        v["Mpixels_per_s"] = round(n / 1e6 / (v["median_ms"] / 1e3), 1)
    r["copy_d2d_cells"]["GBps_read_plus_written"] = round(2 * n * 4 / 1e9 / (r["copy_d2d_cells"]["median_ms"] / 1e3), 1)
    yard = r["interp_first_z_zx_zy"]
    out = {"workload": "etopo1 shape: a FLOAT block of %d x %d cells rendered with ETOPO1.cpt (41 records) on a lattice of %d x %d pixels offset by "
                       "half a cell; ExtractData's light" % (n_rows, n_cols, n_rows, n_cols),
           "method": "HIP events, %d timings per case taken in turn in one process" % REPS,
           "csrc_digest": hipbuild.csrc_digest(), "pixels": n, "block_bytes": int(block.nbytes), "argb_bytes": n * 4, "z_zx_zy_bytes": n * 24,
           "outputs_agree_word_for_word": agree, "cases": r,
           "fused_median_within_yardstick_range": bool(r["render_lattice_shaded"]["median_ms"] <= yard["max_ms"])}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    pal.close()


if __name__ == "__main__":
    main(sys.argv[1:])
