"""What reading a GVRS file image at scattered points costs beside the route through a block: the ETOPO1-shaped INT file image of
tools/file_read_rate.py (12,960 tile records of 120 x 150 cells, a 10,800 x 21,600 grid, shuffled records, extended directory),
1,000,000 points a case.
    python tools/file_points_rate.py [--out profiles/file_points_rate.json] [--tile-rows 90] [--points 1000000] [--reps 20]
HIP events on the context's stream, checksums verified, the timings of a case and of its yardstick taken in turn in one process;
medians, min, max and the spread max - min.  The yardstick of every case is the route the library had before, never the new code:
  (a) a track: the points on a diagonal line across the grid, value and first derivatives.  gf_file_interp_points_dev against
      gf_file_read_block_elems_dev of the bounding rectangle (the whole grid) + gf_block_interp_points_dev
  (b) a scatter: uniformly random points that touch every tile, against the same route
  (c) cells: scattered cells through gf_file_read_points_elems_dev against the whole-grid block read + a gather of the same cells
      with torch indexing on the block (on the context's stream)
max_tiles comes from the host functions, outside the timings (their time is reported).  The aim of (b): the yardstick's median plus
its own spread.  The values are written as they come out; nothing here asserts a rate."""
import ctypes as C
import json
import os
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


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "spread_ms": round(max(v) - min(v), 4), "reps": len(v)}


def _pair(timer, reps, new, old):
    ms = {"points": [], "yardstick": []}
    for _ in range(reps):
        for k, fn in (("yardstick", old), ("points", new)):
            timer.start()
            fn()
            timer.stop()
            ms[k].append(timer.elapsed_ms())
    out = {k: _stats(v) for k, v in ms.items()}
    limit = out["yardstick"]["median_ms"] + out["yardstick"]["spread_ms"]
    out["points_vs_yardstick"] = {"limit_ms": round(limit, 4), "verdict": "within" if out["points"]["median_ms"] <= limit else "ABOVE",
                                  "ratio": round(out["points"]["median_ms"] / out["yardstick"]["median_ms"], 4)}
    return out


def main(argv):
    def opt(name, default):
        return int(argv[argv.index(name) + 1]) if name in argv else default
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    tile_rows, n, reps = opt("--tile-rows", 90), opt("--points", 1000000), opt("--reps", 20)
    import torch
    L = lib()
    ctx = gridfour_amd.GvrsHipContext(0)
    image, grid_shape, want, _, _, _, _, _ = FR.etopo_image(ctx, tile_rows)
    nr, nc = grid_shape
    nt = tile_rows * FR.TILES_ACROSS
    f = gridfour_amd.GvrsFileHip(image)
    rect = np.array((0, 0) + grid_shape, np.int32)
    d_image = DeviceBuffer(ctx, len(image) + 64).fill(0).upload(np.frombuffer(image, np.uint8))
    stream = torch.cuda.ExternalStream(ctx.stream)
    block = torch.empty(nr * nc, dtype=torch.int32, device="cuda")
    p_block = (C.c_void_p * 1)(block.data_ptr())
    d_st, d_pr = DeviceBuffer(ctx, nt * 4), DeviceBuffer(ctx, nt)
    spec = f.points_spec(0, target=gridfour_amd.INTERP_FIRST)
    names = ("z", "zx", "zy", "status")
    rng = np.random.default_rng(21600)

    def block_read():
        check(L.gf_file_read_block_elems_dev(ctx.handle, f._h, d_image.ptr, len(image), _p(rect), 1, p_block, d_st.ptr, d_pr.ptr), "block read")

    def interp_case(rows, cols):
        d_rows, d_cols = DeviceBuffer(ctx, n * 8).upload(rows), DeviceBuffer(ctx, n * 8).upload(cols)
        outs = [{k: DeviceBuffer(ctx, n * (4 if k == "status" else 8)) for k in names} for _ in range(2)]
        o = [_out_struct(_INTERP_OUT, {k: b.ptr for k, b in d.items()}) for d in outs]
        t0 = time.perf_counter()
        touched = f.interp_tiles(spec, rows, cols).size
        host_ms = (time.perf_counter() - t0) * 1e3
        count = C.c_size_t()

        def new():
            check(L.gf_file_interp_points_dev(ctx.handle, f._h, d_image.ptr, len(image), 0, _p(spec), n, d_rows.ptr, d_cols.ptr, None, 1, touched,
                                              _p(o[0]), C.byref(count)), "gf_file_interp_points_dev")

        def old():
            block_read()
            check(L.gf_block_interp_points_dev(ctx.handle, None, _p(spec), C.c_void_p(block.data_ptr()), n, d_rows.ptr, d_cols.ptr, None, _p(o[1])),
                  "gf_block_interp_points_dev")
        new(), old()
        ctx.synchronize()
        assert count.value == touched
        for k in names:
            a, b = (d[k].download(np.int32 if k == "status" else np.uint64, n) for d in outs)
            assert np.array_equal(a, b), k
        r = _pair(gridfour_amd.GpuTimer(ctx), reps, new, old)
        ctx.synchronize()
        r.update(tiles_touched=touched, tiles_total=nt, host_tiles_ms=round(host_ms, 2))
        for d in outs:
            for b in d.values():
                b.free()
        d_rows.free(), d_cols.free()
        return r

    cases = {}
    s = np.linspace(0.0, 1.0, n)
    cases["a_track_interp_first"] = interp_case(s * (nr - 1), s * (nc - 1))
    cases["b_scatter_interp_first"] = interp_case(rng.uniform(0, nr - 1, n), rng.uniform(0, nc - 1, n))

    rows, cols = rng.integers(0, nr, n).astype(np.int32), rng.integers(0, nc, n).astype(np.int32)
    d_rows, d_cols = DeviceBuffer(ctx, n * 4).upload(rows), DeviceBuffer(ctx, n * 4).upload(cols)
    d_val, d_pst = DeviceBuffer(ctx, n * 4), DeviceBuffer(ctx, n * 4)
    p_val = (C.c_void_p * 1)(d_val.ptr.value)
    index = torch.from_numpy(rows.astype(np.int64) * nc + cols).to("cuda")
    t0 = time.perf_counter()
    touched = f.cells_tiles(rows, cols).size
    host_ms = (time.perf_counter() - t0) * 1e3
    count = C.c_size_t()
    gathered = [None]

    def new_cells():
        check(L.gf_file_read_points_elems_dev(ctx.handle, f._h, d_image.ptr, len(image), n, d_rows.ptr, d_cols.ptr, 1, touched, p_val, d_pst.ptr,
                                              C.byref(count)), "gf_file_read_points_elems_dev")

    def old_cells():
        block_read()
        with torch.cuda.stream(stream):
            gathered[0] = block[index]
    new_cells(), old_cells()
    ctx.synchronize()
    assert count.value == touched and not d_pst.download(np.int32, n).any()
    assert np.array_equal(d_val.download(np.int32, n), gathered[0].cpu().numpy()) and np.array_equal(gathered[0].cpu().numpy(), want[rows, cols])
    cases["c_cells"] = _pair(gridfour_amd.GpuTimer(ctx), reps, new_cells, old_cells)
    ctx.synchronize()
    cases["c_cells"].update(tiles_touched=touched, tiles_total=nt, host_tiles_ms=round(host_ms, 2))

    out = {"workload": "etopo1: a file image of %d tile records of %dx%d cells (a %d x %d grid), %d points a case" % ((nt, FR.N_ROWS, FR.N_COLS) + grid_shape + (n,)),
           "codec_ids": FR.IDS, "image_bytes": len(image), "block_bytes": nr * nc * 4,
           "method": "HIP events on the context's stream, %d timings per case and yardstick taken in turn in one process, checksums verified; "
                     "the yardstick is the whole-grid gf_file_read_block_elems_dev + gf_block_interp_points_dev (a, b) or + torch indexing (c)" % reps,
           "csrc_digest": gridfour_amd.build.csrc_digest() if hasattr(gridfour_amd, "build") else None, "cases": cases}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
