"""What reading a block from a file image costs beside the same read from contiguous records: an ETOPO1-shaped INT file image --
12,960 tile records of 120 x 150 cells written by gf_block_write_elems_dev (a 10,800 x 21,600 grid of 90 x 144 tiles; the list
[CodecHuffman, -, -, CodecCanonHuffman], the standard list's integer codecs the device writer takes, at the standard list's
indices), laid in shuffled order with a metadata record in front of every third one behind a header record, and an extended tile
directory (tests/gvrs_file_build.py) -- read as ONE whole-grid block.
    python tools/file_read_rate.py [--out profiles/file_read_rate.json] [--tile-rows 90]
HIP events on the context's stream, checksums verified, 20 timings per case taken in turn in one process; medians, min and max:
  (a) gf_block_read_elems_dev on the records as the writer left them: contiguous, in tile order
  (b) gf_file_read_block_elems_dev on the file image: k_file_locate, the same pipeline with an explicit end per record, k_file_status
  (c) gf_file_read_block_elems_dev on the same image with every fourth directory entry cleared: absent tiles as empty extents
Condition, stated against what is not the code under test:  median(b) <= median(a) + spread(a)  (spread = max - min of that case in
this run): the directory look-up moves 24 bytes a tile in front of a pipeline that moves the tiles.  The values and the verdict are
written as they come out; nothing here asserts them."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gridfour_amd  # noqa: E402
from gridfour_amd import DeviceBuffer, DeviceTileBatch, lib  # noqa: E402
from gridfour_amd._lib import check  # noqa: E402
from gridfour_amd.codec import _ELEM_SPEC  # noqa: E402
import gvrs_file_build as FB  # noqa: E402

REPS = 20
CODECS = [1, 0, 0, 3]
IDS = ["GvrsHuffman", "GvrsDeflate", "GvrsFloat", "GvrsCanonicalHuffman"]
N_ROWS, N_COLS, TILES_ACROSS = 120, 150, 144
FILL = -2 ** 31


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _series(timer, fns):
    ms = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            timer.start()
            fn()
            timer.stop()
            ms[k].append(timer.elapsed_ms())
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "spread_ms": round(max(v) - min(v), 4), "reps": REPS} for k, v in ms.items()}


def etopo_image(ctx, tile_rows=90):
    """The ETOPO1-shaped file image (tools/file_points_rate.py reads it too): (image bytes, the grid's shape, the raster the records
    hold, the tiles' cells [nt, cells], the writer's record blob with its offsets and tile indices and the codec each record used)"""
    nt = tile_rows * TILES_ACROSS
    b = DeviceTileBatch(ctx, N_ROWS, N_COLS, nt, slot_stride=16)
    b.synth_dem(0x9E3779B97F4A7C15 + 2, TILES_ACROSS)
    ctx.synchronize()
    vals = b.get_values().reshape(nt, N_ROWS * N_COLS)
    b.free()
    grid_shape = (tile_rows * N_ROWS, TILES_ACROSS * N_COLS)
    want = vals.reshape(tile_rows, TILES_ACROSS, N_ROWS, N_COLS).transpose(0, 2, 1, 3).reshape(grid_shape)
    master = gridfour_amd.CodecMasterHip(codec_list=CODECS, context=ctx)
    whole = (0, 0) + grid_shape
    idx, blob, off, used, st = master.write_block_dev(N_ROWS, N_COLS, grid_shape, whole, [want], ["int"], raw=True)
    assert not st.any() and sorted(idx.tolist()) == list(range(nt))
    # the file image: the writer's records in shuffled order, a metadata record in front of every third one
    rng = np.random.default_rng(12960)
    records = {int(idx[t]): blob[int(off[t]):int(off[t + 1])].tobytes() for t in range(nt)}
    image, positions = FB.build_image(grid_shape + (N_ROWS, N_COLS), [FB.element("z", "int")], records, codec_ids=IDS,
                                      order=[int(t) for t in rng.permutation(nt)], extended=True,
                                      between=lambda k: FB.other_record(FB.RECORD_METADATA, 64, seed=k) if k % 3 == 0 else b"")
    return image, grid_shape, want, vals, blob, off, idx, used


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    tile_rows = int(argv[argv.index("--tile-rows") + 1]) if "--tile-rows" in argv else 90
    nt = tile_rows * TILES_ACROSS
    L = lib()
    ctx = gridfour_amd.GvrsHipContext(0)
    image, grid_shape, want, vals, blob, off, idx, used = etopo_image(ctx, tile_rows)
    whole = (0, 0) + grid_shape
    total = int(off[nt])
    f = gridfour_amd.GvrsFileHip(image)
    sparse = bytearray(image)
    for t in range(0, nt, 4):
        at, w = FB.entry_offset(image, f.info, t)
        sparse[at:at + w] = bytes(w)
    grid = np.array(grid_shape + (N_ROWS, N_COLS), np.int32)
    rect = np.array(whole, np.int32)
    block_bytes = want.size * 4
    spec = np.zeros(1, _ELEM_SPEC)
    spec["type"], spec["scale"], spec["fill_i"] = 0, 1.0, FILL
    cd = (C.c_int * len(CODECS))(*CODECS)
    d_blob = DeviceBuffer(ctx, total + 64).upload(blob[:total + 64])
    d_off = DeviceBuffer(ctx, off.nbytes).upload(off)
    d_image = DeviceBuffer(ctx, len(image) + 64).fill(0).upload(np.frombuffer(image, np.uint8))
    d_sparse = DeviceBuffer(ctx, len(image) + 64).fill(0).upload(np.frombuffer(bytes(sparse), np.uint8))
    d_block = DeviceBuffer(ctx, block_bytes)
    d_st = DeviceBuffer(ctx, nt * 4)
    d_pr = DeviceBuffer(ctx, nt)
    p_block = (C.c_void_p * 1)(d_block.ptr.value)

    def a_records():
        check(L.gf_block_read_elems_dev(ctx.handle, None, cd, len(CODECS), _p(spec), 1, _p(grid), _p(rect), nt, d_blob.ptr, total, d_off.ptr, 1,
                                        p_block, d_st.ptr), "gf_block_read_elems_dev")

    def b_file():
        check(L.gf_file_read_block_elems_dev(ctx.handle, f._h, d_image.ptr, len(image), _p(rect), 1, p_block, d_st.ptr, d_pr.ptr),
              "gf_file_read_block_elems_dev")

    def c_file_sparse():
        check(L.gf_file_read_block_elems_dev(ctx.handle, f._h, d_sparse.ptr, len(image), _p(rect), 1, p_block, d_st.ptr, d_pr.ptr),
              "gf_file_read_block_elems_dev")

    # every case once outside the timings (the context's buffers grow, code objects load), and the results checked
    for fn, holds in ((a_records, None), (b_file, 1), (c_file_sparse, 0)):
        d_block.fill(0)
        fn()
        ctx.synchronize()
        assert not d_st.download(np.int32, nt).any(), fn.__name__
        got = d_block.download(np.int32, want.size).reshape(grid_shape)
        if holds == 0:
            present = d_pr.download(np.uint8, nt)
            assert present.tolist() == [int(t % 4 != 0) for t in range(nt)]
            tiles = got.reshape(tile_rows, N_ROWS, TILES_ACROSS, N_COLS).transpose(0, 2, 1, 3).reshape(nt, -1)
            assert (tiles[0::4] == FILL).all() and np.array_equal(tiles[1::4], vals[1::4]) and np.array_equal(tiles[3::4], vals[3::4])
        else:
            assert np.array_equal(got, want), fn.__name__
            assert holds is None or d_pr.download(np.uint8, nt).all()
    timer = gridfour_amd.GpuTimer(ctx)
    r = _series(timer, {"a_block_read_elems_dev": a_records, "b_file_read_block_elems_dev": b_file, "c_file_read_quarter_absent": c_file_sparse})
    ctx.synchronize()
    for v in r.values():
        v["GBps_of_block"] = round(block_bytes / 1e9 / (v["median_ms"] / 1e3), 1)
    a, bb = r["a_block_read_elems_dev"], r["b_file_read_block_elems_dev"]
    limit = a["median_ms"] + a["spread_ms"]
    u, c = np.unique(used, return_counts=True)
    out = {"workload": "etopo1: a file image of %d tile records of %dx%d cells, read as one block of %d x %d cells" % ((nt, N_ROWS, N_COLS) + grid_shape),
           "codec_list": CODECS, "codec_ids": IDS, "method": "HIP events, %d timings per case taken in turn in one process, checksums verified" % REPS,
           "csrc_digest": gridfour_amd.build.csrc_digest() if hasattr(gridfour_amd, "build") else None,
           "records": nt, "record_bytes": total, "image_bytes": len(image), "directory": "extended", "block_bytes": block_bytes,
           "winners": {int(x): int(n) for x, n in zip(u, c)}, "cases": r,
           "conditions": {"b_le_a_plus_spread_a": {"value_ms": bb["median_ms"], "limit_ms": round(limit, 4), "holds": bool(bb["median_ms"] <= limit)}}}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
