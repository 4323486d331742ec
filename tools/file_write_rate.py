"""What writing a file image costs beside writing the same records into a plain blob: an ETOPO1-shaped INT block -- a 10,800 x
21,600 grid of 90 x 144 tiles of 120 x 150 cells, 12,960 tile records, the list [CodecHuffman] -- written as ONE whole-grid block.
    python tools/file_write_rate.py [--out profiles/file_write_rate.json] [--tile-rows 90]
HIP events on the context's stream, checksums on, 20 timings per case taken in turn in one process; medians, min and max:
  (a) gf_block_write_elems_dev on the block into a plain blob (the yardstick: it exists without the file writer)
  (b) gf_file_write_block_elems_dev on the same block: the same pipeline writing the records straight into the image, around it the
      upload of the header record, k_file_dir_rect, k_file_dir_entries, k_file_dir_crc and k_file_finish
  (c) a device-to-device copy of the bytes the file form adds (header record, tile directory), where the HIP runtime can be loaded
Aim, stated against what is not the code under test:  median(b) <= median(a) + spread(a) + median(c)  (spread = max - min of that
case in this run).  The image is read back once, opened and compared with gf_file_assemble over the records of (a).  The values
and the verdict are written as they come out; nothing here asserts them."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gridfour_amd  # noqa: E402
from gridfour_amd import DeviceBuffer, DeviceTileBatch, GvrsFileFacts, GvrsFileHip, lib  # noqa: E402
from gridfour_amd._lib import check  # noqa: E402

REPS = 20
IDS = ["GvrsHuffman"]
CODECS = [1]
N_ROWS, N_COLS, TILES_ACROSS = 120, 150, 144


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


def _hip_copy(ctx, dst, src, n):
    """a function that enqueues a device-to-device copy of n bytes on the context's stream, or None without the HIP runtime"""
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        return None
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = lib().gf_context_stream(ctx.handle)

    def copy():
        assert hip.hipMemcpyAsync(dst, src, n, 3, stream) == 0          # hipMemcpyDeviceToDevice
    return copy


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    tile_rows = int(argv[argv.index("--tile-rows") + 1]) if "--tile-rows" in argv else 90
    nt = tile_rows * TILES_ACROSS
    L = lib()
    ctx = gridfour_amd.GvrsHipContext(0)
    b = DeviceTileBatch(ctx, N_ROWS, N_COLS, nt, slot_stride=16)
    b.synth_dem(0x9E3779B97F4A7C15 + 2, TILES_ACROSS)
    ctx.synchronize()
    vals = b.get_values().reshape(nt, N_ROWS * N_COLS)
    b.free()
    grid_shape = (tile_rows * N_ROWS, TILES_ACROSS * N_COLS)
    block = np.ascontiguousarray(vals.reshape(tile_rows, TILES_ACROSS, N_ROWS, N_COLS).transpose(0, 2, 1, 3).reshape(grid_shape))
    del vals
    facts = GvrsFileFacts(grid_shape + (N_ROWS, N_COLS), ["int"], codec_ids=IDS, elem_facts=[dict(name="z", label="elevation", unit="m")],
                          product_label="ETOPO1-shaped", metadata=[("GvrsJavaCodecs", 0, 6, b"GvrsHuffman, org.gridfour.compress.CodecHuffman", "codecs")])
    first, most = facts.plan()
    rect = np.array((0, 0) + grid_shape, np.int32)
    grid = np.array(grid_shape + (N_ROWS, N_COLS), np.int32)
    cd = (C.c_int * len(CODECS))(*CODECS)
    full = nt * int(L.gf_tile_record_max_bytes_elems(_p(facts.specs), 1, N_ROWS, N_COLS))
    d_block = DeviceBuffer(ctx, block.nbytes + 16).upload(block)
    p_block = (C.c_void_p * 1)(d_block.ptr.value)
    d_blob = DeviceBuffer(ctx, full + 64)
    d_off = DeviceBuffer(ctx, (nt + 1) * 8)
    d_image = DeviceBuffer(ctx, most + 64)
    d_idx, d_st, d_used = DeviceBuffer(ctx, nt * 4), DeviceBuffer(ctx, nt * 4), DeviceBuffer(ctx, nt)
    d_bytes, d_fst = DeviceBuffer(ctx, 16), DeviceBuffer(ctx, 16)

    def a_block_write():
        check(L.gf_block_write_elems_dev(ctx.handle, None, cd, len(CODECS), _p(facts.specs), None, 1, _p(grid), _p(rect), p_block, 0, None, 0, None,
                                         0, 1, d_blob.ptr, full, d_off.ptr, d_idx.ptr, d_used.ptr, d_st.ptr), "gf_block_write_elems_dev")

    def b_file_write():
        check(L.gf_file_write_block_elems_dev(ctx.handle, *facts.args(), _p(rect), p_block, 0, d_image.ptr, most, d_bytes.ptr, d_fst.ptr, d_idx.ptr,
                                              d_st.ptr, d_used.ptr), "gf_file_write_block_elems_dev")

    # both once outside the timings (the context's buffers grow, code objects load), and the results checked against each other
    a_block_write()
    ctx.synchronize()
    off = d_off.download(np.uint64, nt + 1)
    idx = d_idx.download(np.int32, nt)
    assert not d_st.download(np.int32, nt).any()
    total = int(off[nt])
    blob = d_blob.download(np.uint8, total)
    b_file_write()
    ctx.synchronize()
    assert int(d_fst.download(np.int32, 1)[0]) == 0 and not d_st.download(np.int32, nt).any()
    image_bytes = int(d_bytes.download(np.uint64, 1)[0])
    image = d_image.download(np.uint8, image_bytes).tobytes()
    records = [blob[int(off[t]):int(off[t + 1])].tobytes() for t in range(nt)]
    assert image == GvrsFileHip.assemble(facts, records, idx), "the device form's image differs from gf_file_assemble"
    f = GvrsFileHip(image)
    assert f.info["dir_n_rows"] * f.info["dir_n_cols"] == nt and f.tile_position(0) == first + 8
    added = image_bytes - total
    del records, blob
    fns = {"a_block_write_elems_dev": a_block_write, "b_file_write_block_elems_dev": b_file_write}
    copy = _hip_copy(ctx, d_blob.ptr, d_image.ptr, added)
    if copy is not None:
        fns["c_copy_of_added_bytes"] = copy
    timer = gridfour_amd.GpuTimer(ctx)
    r = _series(timer, fns)
    ctx.synchronize()
    a, bb = r["a_block_write_elems_dev"], r["b_file_write_block_elems_dev"]
    c_ms = r["c_copy_of_added_bytes"]["median_ms"] if copy is not None else 0.0
    limit = a["median_ms"] + a["spread_ms"] + c_ms
    for v in (a, bb):
        v["GBps_of_block"] = round(block.nbytes / 1e9 / (v["median_ms"] / 1e3), 1)
    out = {"workload": "etopo1: one block of %d x %d INT cells written as %d tile records of %dx%d cells" % (grid_shape + (nt, N_ROWS, N_COLS)),
           "codec_ids": IDS, "method": "HIP events, %d timings per case taken in turn in one process, checksums on" % REPS,
           "csrc_digest": gridfour_amd.build.csrc_digest() if hasattr(gridfour_amd, "build") else None,
           "records": nt, "record_bytes": total, "image_bytes": image_bytes, "added_bytes": added, "block_bytes": int(block.nbytes),
           "directory_entries": nt, "cases": r, "extra_ms_b_minus_a": round(bb["median_ms"] - a["median_ms"], 4),
           "conditions": {"b_le_a_plus_spread_a_plus_copy": {"value_ms": bb["median_ms"], "limit_ms": round(limit, 4),
                                                             "holds": bool(bb["median_ms"] <= limit)}}}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
