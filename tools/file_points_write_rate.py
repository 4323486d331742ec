"""What writing a GVRS file image at scattered points costs beside the only route the library had before: the ETOPO1-shaped INT
raster of tools/file_read_rate.py (12,960 tiles of 120 x 150 cells, a 10,800 x 21,600 grid, shuffled records, extended directory)
in a file whose codec list the device record writer takes (GvrsHuffman, GvrsCanonicalHuffman), 1,000,000 points a case.
    python tools/file_points_write_rate.py [--out profiles/file_points_write_rate.json] [--tile-rows 90] [--points 1000000] [--reps 20]
                                           [--once]        (one call of each route per case and no timing: for a kernel trace)
                                           [--case a|b]    (one case alone)   [--route points|yardstick]   (with --once: one route alone)
HIP events on the context's stream, the timings of a case and of its yardstick taken in turn in one process; medians, min, max and
the spread max - min.  Before every timing the working image is restored from the old one on the same stream, outside the events.
The yardstick is gf_file_read_block_elems_dev of the whole grid + a torch scatter of the values into the block +
gf_file_update_block_elems_dev of the whole grid:
  (a) a track: the cells on a diagonal line across the grid (about 250 tiles touched)
  (b) a scatter: uniformly random cells that touch every tile
max_tiles and the image's room come from the host functions, outside the timings (their time is reported).  The aim: the
yardstick's median plus its own spread.  The values are written as they come out; nothing here asserts a rate."""
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
from gridfour_amd import DeviceBuffer, DeviceTileBatch, lib  # noqa: E402
from gridfour_amd._lib import check  # noqa: E402
import file_read_rate as FR  # noqa: E402
import gvrs_file_build as FB  # noqa: E402
from file_points_rate import _p, _stats  # noqa: E402

IDS, CODECS = ["GvrsHuffman", "GvrsCanonicalHuffman"], [gridfour_amd.CODEC_HUFFMAN, gridfour_amd.CODEC_CANON_HUFFMAN]
TIME = 1_700_000_000_123


def etopo_image(ctx, tile_rows):
    """FR.etopo_image's raster and layout under a codec list the device record writer takes -> (image bytes, the grid's shape)"""
    nt = tile_rows * FR.TILES_ACROSS
    b = DeviceTileBatch(ctx, FR.N_ROWS, FR.N_COLS, nt, slot_stride=16)
    b.synth_dem(0x9E3779B97F4A7C15 + 2, FR.TILES_ACROSS)
    ctx.synchronize()
    vals = b.get_values().reshape(nt, FR.N_ROWS * FR.N_COLS)
    b.free()
    grid_shape = (tile_rows * FR.N_ROWS, FR.TILES_ACROSS * FR.N_COLS)
    want = vals.reshape(tile_rows, FR.TILES_ACROSS, FR.N_ROWS, FR.N_COLS).transpose(0, 2, 1, 3).reshape(grid_shape)
    master = gridfour_amd.CodecMasterHip(codec_list=CODECS, context=ctx)
    idx, blob, off, used, st = master.write_block_dev(FR.N_ROWS, FR.N_COLS, grid_shape, (0, 0) + grid_shape, [want], ["int"], raw=True)
    assert not st.any() and sorted(idx.tolist()) == list(range(nt))
    rng = np.random.default_rng(12960)
    records = {int(idx[t]): blob[int(off[t]):int(off[t + 1])].tobytes() for t in range(nt)}
    image, _ = FB.build_image(grid_shape + (FR.N_ROWS, FR.N_COLS), [FB.element("z", "int")], records, codec_ids=IDS,
                              order=[int(t) for t in rng.permutation(nt)], extended=True,
                              between=lambda k: FB.other_record(FB.RECORD_METADATA, 64, seed=k) if k % 3 == 0 else b"")
    return image, grid_shape


def main(argv):
    def opt(name, default):
        return int(argv[argv.index(name) + 1]) if name in argv else default
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    tile_rows, n, reps, once = opt("--tile-rows", 90), opt("--points", 1000000), opt("--reps", 20), "--once" in argv
    import torch
    L = lib()
    ctx = gridfour_amd.GvrsHipContext(0)
    image, grid_shape = etopo_image(ctx, tile_rows)
    nr, nc = grid_shape
    nt = tile_rows * FR.TILES_ACROSS
    f = gridfour_amd.GvrsFileHip(image)
    u = f.update_begin()
    cap = u.plan()[0]
    rect = np.array((0, 0) + grid_shape, np.int32)
    stream = torch.cuda.ExternalStream(ctx.stream)
    old_image = torch.from_numpy(np.frombuffer(image, np.uint8).copy()).to("cuda")
    work = [torch.zeros(cap + 64, dtype=torch.uint8, device="cuda") for _ in range(2)]          # the points route's image, the yardstick's
    block = torch.empty(nr * nc, dtype=torch.int32, device="cuda")
    p_block = (C.c_void_p * 1)(block.data_ptr())
    d_st, d_pr = DeviceBuffer(ctx, nt * 4), DeviceBuffer(ctx, nt)
    d_bytes, d_fst = [DeviceBuffer(ctx, 16) for _ in range(2)], [DeviceBuffer(ctx, 16) for _ in range(2)]
    d_idx, d_tst = [DeviceBuffer(ctx, nt * 4 + 16) for _ in range(2)], [DeviceBuffer(ctx, nt * 4 + 16) for _ in range(2)]
    rng = np.random.default_rng(21600)

    def restore(k):
        with torch.cuda.stream(stream):
            work[k][:len(image)].copy_(old_image)

    def case(rows, cols):
        rows, cols = rows.astype(np.int32), cols.astype(np.int32)
        cell, first = np.unique(rows.astype(np.int64) * nc + cols, return_index=True)       # the last point of a cell wins: keep distinct cells, so
        rows, cols = rows[np.sort(first)], cols[np.sort(first)]                              # that the torch scatter of the yardstick says the same
        m = rows.size
        values = rng.integers(-10000, 9000, m).astype(np.int32)
        d_rows, d_cols, d_val = (DeviceBuffer(ctx, m * 4 + 16).upload(a) for a in (rows, cols, values))
        p_val = (C.c_void_p * 1)(d_val.ptr.value)
        d_pst = DeviceBuffer(ctx, m * 4 + 16)
        index = torch.from_numpy(rows.astype(np.int64) * nc + cols).to("cuda")
        t_values = torch.from_numpy(values).to("cuda")
        t0 = time.perf_counter()
        touched = f.cells_tiles(rows, cols).size
        host_ms = (time.perf_counter() - t0) * 1e3
        count = C.c_size_t()

        def new():
            check(L.gf_file_update_points_elems_dev(ctx.handle, u.handle, m, d_rows.ptr, d_cols.ptr, p_val, touched, 0, TIME, C.c_void_p(work[0].data_ptr()),
                                                    cap, d_bytes[0].ptr, d_fst[0].ptr, d_pst.ptr, d_idx[0].ptr, d_tst[0].ptr, None, C.byref(count)),
                  "gf_file_update_points_elems_dev")

        def old():
            check(L.gf_file_read_block_elems_dev(ctx.handle, f._h, C.c_void_p(work[1].data_ptr()), len(image), _p(rect), 1, p_block, d_st.ptr, d_pr.ptr),
                  "gf_file_read_block_elems_dev")
            with torch.cuda.stream(stream):
                block[index] = t_values
            check(L.gf_file_update_block_elems_dev(ctx.handle, u.handle, _p(rect), p_block, 0, TIME, C.c_void_p(work[1].data_ptr()), cap, d_bytes[1].ptr,
                                                   d_fst[1].ptr, d_idx[1].ptr, d_tst[1].ptr, None), "gf_file_update_block_elems_dev")
        if once:                                                   # a kernel trace: the chosen route alone, run once, nothing read back
            route = argv[argv.index("--route") + 1] if "--route" in argv else "both"
            restore(0), restore(1)
            if route in ("points", "both"):
                new()
            if route in ("yardstick", "both"):
                old()
            ctx.synchronize()
            return {"points": m, "tiles_touched": touched, "route": route}
        restore(0), restore(1)
        new(), old()
        ctx.synchronize()
        assert count.value == touched and not d_pst.download(np.int32, m).any()
        sizes = [int(b.download(np.uint64, 1)[0]) for b in d_bytes]
        assert [int(b.download(np.int32, 1)[0]) for b in d_fst] == [0, 0]
        assert not d_tst[0].download(np.int32, touched).any() and not d_tst[1].download(np.int32, nt).any()
        # both images hold the old raster with the points' values: read the cells back from each
        for k in range(2):
            g = gridfour_amd.GvrsFileHip(work[k][:sizes[k]].cpu().numpy())
            d_got, d_gst = DeviceBuffer(ctx, m * 4 + 16), DeviceBuffer(ctx, m * 4 + 16)
            c2 = C.c_size_t()
            check(L.gf_file_read_points_elems_dev(ctx.handle, g._h, C.c_void_p(work[k].data_ptr()), sizes[k], m, d_rows.ptr, d_cols.ptr, 1, touched,
                                                  (C.c_void_p * 1)(d_got.ptr.value), d_gst.ptr, C.byref(c2)), "read back")
            ctx.synchronize()
            assert np.array_equal(d_got.download(np.int32, m), values) and not d_gst.download(np.int32, m).any()
            d_got.free(), d_gst.free()
        same = sizes[0] == sizes[1] and bool(torch.equal(work[0][:sizes[0]], work[1][:sizes[1]]))
        r = {"points": m, "tiles_touched": touched, "tiles_total": nt, "host_tiles_ms": round(host_ms, 2), "image_bytes_after": sizes,
             "images_equal": same}
        if not once:
            timer = gridfour_amd.GpuTimer(ctx)
            ms = {"points": [], "yardstick": []}
            for _ in range(reps):
                for k, (name, fn) in enumerate((("points", new), ("yardstick", old))):
                    restore(k)
                    timer.start()
                    fn()
                    timer.stop()
                    ms[name].append(timer.elapsed_ms())
            r.update({k: _stats(v) for k, v in ms.items()})
            limit = r["yardstick"]["median_ms"] + r["yardstick"]["spread_ms"]
            r["points_vs_yardstick"] = {"limit_ms": round(limit, 4), "verdict": "within" if r["points"]["median_ms"] <= limit else "ABOVE the aim",
                                        "ratio": round(r["points"]["median_ms"] / r["yardstick"]["median_ms"], 4)}
        ctx.synchronize()
        for b in (d_rows, d_cols, d_val, d_pst):
            b.free()
        return r

    cases = {}
    s = np.linspace(0.0, 1.0, n)
    only = argv[argv.index("--case") + 1] if "--case" in argv else "ab"
    if "a" in only:
        cases["a_track"] = case(np.floor(s * (nr - 1)), np.floor(s * (nc - 1)))
    if "b" in only:
        cases["b_scatter"] = case(rng.integers(0, nr, n), rng.integers(0, nc, n))
    out = {"workload": "etopo1: a file image of %d tile records of %dx%d cells (a %d x %d grid), %d points a case (distinct cells kept)"
                       % ((nt, FR.N_ROWS, FR.N_COLS) + grid_shape + (n,)),
           "codec_ids": IDS, "image_bytes": len(image), "block_bytes": nr * nc * 4, "image_room_bytes": cap,
           "method": "HIP events on the context's stream, %d timings per case and yardstick taken in turn in one process, the working image "
                     "restored before each outside the events; the yardstick is the whole-grid gf_file_read_block_elems_dev + a torch scatter + "
                     "the whole-grid gf_file_update_block_elems_dev" % reps,
           "csrc_digest": gridfour_amd.build.csrc_digest() if hasattr(gridfour_amd, "build") else None, "cases": cases}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
