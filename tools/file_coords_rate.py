"""What querying a GVRS file image at longitude / latitude costs beside the two calls it fuses: the ETOPO1-shaped INT file image of
tools/file_read_rate.py (12,960 tile records of 120 x 150 cells, a 10,800 x 21,600 grid, shuffled records, extended directory),
its header given geographic coordinates over the whole globe (one arc minute a cell: the longitudes wrap), 1,000,000 points a case.
    python tools/file_coords_rate.py [--out profiles/file_coords_rate.json] [--tile-rows 90] [--points 1000000] [--reps 20]
HIP events on the context's stream, checksums verified, value and first derivatives with the file's column-spacing rule; the
timings of the fused call, of its yardstick and of the mapping are taken in turn in one process; medians, min, max and the spread
max - min.  THE YARDSTICK is the unfused route on the entry point the library had before: gf_file_interp_points_dev on rows,
columns and spacings that gf_file_map_points_dev mapped beforehand, outside its timing.  THE AIM for the fused call
gf_file_interp_coords_dev: the yardstick's median plus the median of gf_file_map_points_dev on the same points (fusing is only
worth having if it does not lose to the two calls it replaces) plus the yardstick's own spread.
  (a) a track: the points on a great diagonal from the south-west to the north-east
  (b) a scatter: uniformly random longitudes (a turn beyond either end included: the retries run) and latitudes
max_tiles comes from the host function, outside the timings (its time is reported).  The fused call's outputs are compared with
the yardstick's bit for bit before anything is timed.  The values are written as they come out; nothing here asserts a rate."""
import ctypes as C
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gridfour_amd  # noqa: E402
from gridfour_amd import DeviceBuffer, lib  # noqa: E402
from gridfour_amd._lib import check  # noqa: E402
from gridfour_amd.codec import _INTERP_OUT, _out_struct  # noqa: E402
import file_read_rate as FR  # noqa: E402
import gvrs_file_build as FB  # noqa: E402


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "spread_ms": round(max(v) - min(v), 4), "reps": len(v)}


def geographic(image, grid_shape):
    """the image with its header stating geographic coordinates over the globe (the fields of gvrs_file_build.header_record)"""
    nr, nc = grid_shape
    cell_x, cell_y = 360.0 / nc, 180.0 / nr
    x0, y0 = -180.0, -90.0 + cell_y / 2
    x1, y1 = x0 + (nc - 1) * cell_x, y0 + (nr - 1) * cell_y
    b = bytearray(image)
    b[130] = 2
    struct.pack_into("<18d", b, 136, x0, y0, x1, y1, cell_x, cell_y, 1 / cell_x, 0.0, -x0 / cell_x, 0.0, 1 / cell_y, -y0 / cell_y,
                     cell_x, 0.0, x0, 0.0, cell_y, y0)
    return FB.refresh_header_crc(bytes(b))


def main(argv):
    def opt(name, default):
        return int(argv[argv.index(name) + 1]) if name in argv else default
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    tile_rows, n, reps = opt("--tile-rows", 90), opt("--points", 1000000), opt("--reps", 20)
    L = lib()
    ctx = gridfour_amd.GvrsHipContext(0)
    image, grid_shape, _, _, _, _, _, _ = FR.etopo_image(ctx, tile_rows)
    image = geographic(image, grid_shape)
    nt = tile_rows * FR.TILES_ACROSS
    f = gridfour_amd.GvrsFileHip(image)
    assert f.info["coordinate_system"] == 2
    spec = f.coords_spec(0, gridfour_amd.INTERP_FIRST)
    assert int(spec["wrap"][0]) == 1
    d_image = DeviceBuffer(ctx, len(image) + 64).fill(0).upload(np.frombuffer(image, np.uint8))
    names = ("z", "zx", "zy", "status")
    rng = np.random.default_rng(21600)
    kind, to_grid = gridfour_amd.COORDS_FILE, gridfour_amd.MAP_GEO_TO_GRID

    def case(lon, lat):
        d_lon, d_lat = DeviceBuffer(ctx, n * 8).upload(lon), DeviceBuffer(ctx, n * 8).upload(lat)
        d_rows, d_cols, d_cs, d_used = (DeviceBuffer(ctx, n * 8) for _ in range(4))
        outs = [{k: DeviceBuffer(ctx, n * (4 if k == "status" else 8)) for k in names} for _ in range(2)]
        o = [_out_struct(_INTERP_OUT, {k: b.ptr for k, b in d.items()}) for d in outs]
        t0 = time.perf_counter()
        touched = f.interp_coords_tiles(kind, spec, lon, lat).size
        host_ms = (time.perf_counter() - t0) * 1e3
        count = [C.c_size_t(), C.c_size_t()]

        def mapping():
            check(L.gf_file_map_points_dev(ctx.handle, f._h, to_grid, n, d_lon.ptr, d_lat.ptr, d_rows.ptr, d_cols.ptr, None, None, d_cs.ptr, None),
                  "gf_file_map_points_dev")

        def fused():
            check(L.gf_file_interp_coords_dev(ctx.handle, f._h, d_image.ptr, len(image), 0, kind, _p(spec), n, d_lon.ptr, d_lat.ptr, None, 1, touched,
                                              _p(o[0]), d_used.ptr, C.byref(count[0])), "gf_file_interp_coords_dev")

        def yardstick():
            check(L.gf_file_interp_points_dev(ctx.handle, f._h, d_image.ptr, len(image), 0, _p(spec), n, d_rows.ptr, d_cols.ptr, d_cs.ptr, 1, touched,
                                              _p(o[1]), C.byref(count[1])), "gf_file_interp_points_dev")
        mapping(), fused(), yardstick()
        ctx.synchronize()
        assert count[0].value == count[1].value == touched
        for k in names:
            a, b = (d[k].download(np.int32 if k == "status" else np.uint64, n) for d in outs)
            assert np.array_equal(a, b), k
        assert np.array_equal(d_used.download(np.uint64, n), d_cs.download(np.uint64, n))
        timer = gridfour_amd.GpuTimer(ctx)
        ms = {"yardstick": [], "fused": [], "mapping": []}
        for _ in range(reps):
            for k, fn in (("yardstick", yardstick), ("fused", fused), ("mapping", mapping)):
                timer.start()
                fn()
                timer.stop()
                ms[k].append(timer.elapsed_ms())
        ctx.synchronize()
        r = {k: _stats(v) for k, v in ms.items()}
        limit = r["yardstick"]["median_ms"] + r["mapping"]["median_ms"] + r["yardstick"]["spread_ms"]
        r["fused_vs_aim"] = {"limit_ms": round(limit, 4), "verdict": "within" if r["fused"]["median_ms"] <= limit else "ABOVE",
                             "fused_over_yardstick": round(r["fused"]["median_ms"] / r["yardstick"]["median_ms"], 4),
                             "fused_over_the_two_calls": round(r["fused"]["median_ms"] / (r["yardstick"]["median_ms"] + r["mapping"]["median_ms"]), 4)}
        st = outs[0]["status"].download(np.int32, n)
        r.update(tiles_touched=touched, tiles_total=nt, host_tiles_ms=round(host_ms, 2), points_ok=int((st == 0).sum()))
        for d in outs:
            for b in d.values():
                b.free()
        for b in (d_lon, d_lat, d_rows, d_cols, d_cs, d_used):
            b.free()
        return r

    cases = {}
    s = np.linspace(0.0, 1.0, n)
    cases["a_track"] = case(-180.0 + 359.9 * s, -89.9 + 179.8 * s)
    cases["b_scatter"] = case(rng.uniform(-540.0, 540.0, n), rng.uniform(-90.0, 90.0, n))
    out = {"workload": "etopo1: a geographic file image of %d tile records of %dx%d cells (a %d x %d grid), %d points a case, value and first "
                       "derivatives" % ((nt, FR.N_ROWS, FR.N_COLS) + grid_shape + (n,)),
           "codec_ids": FR.IDS, "image_bytes": len(image),
           "method": "HIP events on the context's stream, %d timings of yardstick, fused call and mapping taken in turn in one process, checksums "
                     "verified; the yardstick is gf_file_interp_points_dev on rows, columns and spacings mapped beforehand" % reps,
           "csrc_digest": gridfour_amd.build.csrc_digest() if hasattr(gridfour_amd, "build") else None, "cases": cases}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
