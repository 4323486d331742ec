"""What a block read costs beside the decode it is built on and beside a plain copy of the block's bytes: the ETOPO1-shaped batch
of tools/codec_master_rate.py --device-records (12,960 tile records of 120 x 150 cells: a 10,800 x 21,600 grid of 90 x 144 tiles)
read as ONE whole-grid block, once as an INT element and once as a SHORT element.
    python tools/block_read_rate.py [--out profiles/block_read_rate.json] [--tile-rows 90]
HIP events on the context's stream, checksums verified, 20 timings per case taken in turn in one process; medians, min and max:
  (a) gf_tile_record_decode_batch_elems_dev alone (every eighth record is in standard form: the scatter route, as the block read takes)
  (b) a device-to-device hipMemcpyAsync of the block's bytes
  (c) gf_block_read_elems_dev
  (d) gf_block_from_tiles_dev alone, on the decoded tiles of (a)
  (e) gf_tiles_from_block_dev alone, back into tiles
Conditions, stated against what is not the code under test:  median(c) <= median(a) + median(b) + spread(a);  median(d) and
median(e) <= median(b) + spread(b)  (spread = max - min of that case in this run).  The values and the verdicts are written as
they come out; nothing here asserts them."""
import ctypes as C
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gridfour_amd  # noqa: E402
from gridfour_amd import DeviceBuffer, DeviceTileBatch, lib  # noqa: E402
from gridfour_amd._lib import check  # noqa: E402
from gridfour_amd.codec import _ELEM_SPEC  # noqa: E402

REPS = 20
CODECS = [1, 2, 0, 3]
N_ROWS, N_COLS, TILES_ACROSS = 120, 150, 144


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("libamdhip64 not loadable")


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


def one_element(L, hip, ctx, timer, kind, vals, tile_rows):
    nt, cells = vals.shape
    short = kind == "short"
    item = 2 if short else 4
    dtype = np.int16 if short else np.int32
    fill = -32768 if short else -2 ** 31
    src = np.clip(vals, -32767, 32767).astype(np.int16) if short else vals
    cd = (C.c_int * len(CODECS))(*CODECS)
    cap = nt * int(L.gf_tile_record_max_bytes(int(short), N_ROWS, N_COLS))
    blob = np.empty(cap, np.uint8)
    off = np.zeros(nt + 1, np.uint64)
    idx = np.arange(nt, dtype=np.int32)
    used = np.zeros(nt, np.uint8)
    check(L.gf_tile_record_encode_batch(ctx.handle, cd, len(CODECS), int(short), fill, N_ROWS, N_COLS, nt, _p(idx), _p(src), 1, _p(blob), cap,
                                        _p(off), _p(used)), "gf_tile_record_encode_batch")
    # every eighth record in standard form (the cells themselves): the records then name more than one class, and an INT element
    # too takes the driver's scatter route (temporary, then k_elem_scatter) in (a) as in (c)
    recs = [bytes(blob[int(off[t]):int(off[t + 1])]) for t in range(nt)]
    raw = src.astype("<i2" if short else "<i4")
    for t in range(0, nt, 8):
        el = raw[t].tobytes()
        size = (8 + len(el) + 12 + 7) // 8 * 8
        r = bytearray(size)
        struct.pack_into("<iB3xii", r, 0, size, 2, t, len(el))
        r[16:16 + len(el)] = el
        struct.pack_into("<I", r, size - 4, L.gf_crc32c(C.c_char_p(bytes(r[:size - 4])), size - 4))
        recs[t] = bytes(r)
        used[t] = 255
    off[1:] = np.cumsum([len(r) for r in recs])
    blob = np.frombuffer(b"".join(recs) + b"\0" * 64, np.uint8)
    total = int(off[nt])
    u, c = np.unique(used, return_counts=True)
    grid = np.array([tile_rows * N_ROWS, TILES_ACROSS * N_COLS, N_ROWS, N_COLS], np.int32)
    rect = np.array([0, 0, grid[0], grid[1]], np.int32)
    block_bytes = int(grid[0]) * int(grid[1]) * item
    spec = np.zeros(1, _ELEM_SPEC)
    spec["type"], spec["scale"], spec["fill_i"] = int(short), 1.0, fill
    d_blob = DeviceBuffer(ctx, total + 64).upload(blob[:total + 64])
    d_off = DeviceBuffer(ctx, off.nbytes).upload(off)
    d_idx = DeviceBuffer(ctx, nt * 4)
    d_tiles = DeviceBuffer(ctx, nt * cells * item)
    d_block = DeviceBuffer(ctx, block_bytes)
    d_copy = DeviceBuffer(ctx, block_bytes)
    d_back = DeviceBuffer(ctx, nt * cells * item)
    d_st = DeviceBuffer(ctx, nt * 4)
    p_tiles, p_block = (C.c_void_p * 1)(d_tiles.ptr.value), (C.c_void_p * 1)(d_block.ptr.value)
    stream = C.c_void_p(ctx.stream)
    fill_bits = fill & 0xffffffff
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

    def a_decode():
        check(L.gf_tile_record_decode_batch_elems_dev(ctx.handle, None, cd, len(CODECS), _p(spec), 1, N_ROWS, N_COLS, nt, d_blob.ptr, total,
                                                      d_off.ptr, 1, d_idx.ptr, p_tiles, d_st.ptr), "gf_tile_record_decode_batch_elems_dev")

    def b_copy():
        assert hip.hipMemcpyAsync(d_copy.ptr, d_block.ptr, block_bytes, 3, stream) == 0           # hipMemcpyDeviceToDevice

    def c_block_read():
        check(L.gf_block_read_elems_dev(ctx.handle, None, cd, len(CODECS), _p(spec), 1, _p(grid), _p(rect), nt, d_blob.ptr, total, d_off.ptr, 1,
                                        p_block, d_st.ptr), "gf_block_read_elems_dev")

    def d_gather():
        check(L.gf_block_from_tiles_dev(ctx.handle, None, _p(grid), _p(rect), int(short), fill_bits, nt, d_idx.ptr, None, d_tiles.ptr,
                                        d_block.ptr), "gf_block_from_tiles_dev")

    def e_cut():
        check(L.gf_tiles_from_block_dev(ctx.handle, None, _p(grid), _p(rect), int(short), fill_bits, 0, d_block.ptr, nt, d_idx.ptr, d_back.ptr,
                                        None), "gf_tiles_from_block_dev")

    # every case once outside the timings (the context's buffers grow, code objects load), and the results checked
    want = src.reshape(tile_rows, TILES_ACROSS, N_ROWS, N_COLS).transpose(0, 2, 1, 3).reshape(int(grid[0]), int(grid[1]))
    a_decode()
    ctx.synchronize()
    assert (d_st.download(np.int32, nt) == 0).all() and np.array_equal(d_idx.download(np.int32, nt), idx)
    assert np.array_equal(d_tiles.download(dtype, nt * cells).reshape(nt, cells), src)
    c_block_read()
    ctx.synchronize()
    assert (d_st.download(np.int32, nt) == 0).all()
    assert np.array_equal(d_block.download(dtype, want.size).reshape(want.shape), want), "gf_block_read_elems_dev"
    d_block.fill(0)
    d_gather()
    ctx.synchronize()
    assert np.array_equal(d_block.download(dtype, want.size).reshape(want.shape), want), "gf_block_from_tiles_dev"
    e_cut()
    b_copy()
    ctx.synchronize()
    assert np.array_equal(d_back.download(dtype, nt * cells).reshape(nt, cells), src), "gf_tiles_from_block_dev"
    r = _series(timer, {"a_decode_elems_dev": a_decode, "b_copy_d2d": b_copy, "c_block_read_elems_dev": c_block_read,
                        "d_block_from_tiles_dev": d_gather, "e_tiles_from_block_dev": e_cut})
    ctx.synchronize()
    a, b, c_, d, e = (r[k] for k in ("a_decode_elems_dev", "b_copy_d2d", "c_block_read_elems_dev", "d_block_from_tiles_dev", "e_tiles_from_block_dev"))
    for v in r.values():
        v["GBps_of_block"] = round(block_bytes / 1e9 / (v["median_ms"] / 1e3), 1)
    limit_c = a["median_ms"] + b["median_ms"] + a["spread_ms"]
    limit_de = b["median_ms"] + b["spread_ms"]
    out = {"element": kind, "records": nt, "record_bytes": total, "block": [int(grid[0]), int(grid[1])], "block_bytes": block_bytes,
           "winners": {int(x): int(n) for x, n in zip(u, c)}, "scatter_route": bool(short or len(u) > 1), "cases": r,      # (winner 255: standard form)
           "conditions": {
               "c_le_a_plus_b_plus_spread_a": {"value_ms": c_["median_ms"], "limit_ms": round(limit_c, 4), "holds": bool(c_["median_ms"] <= limit_c)},
               "d_le_b_plus_spread_b": {"value_ms": d["median_ms"], "limit_ms": round(limit_de, 4), "holds": bool(d["median_ms"] <= limit_de)},
               "e_le_b_plus_spread_b": {"value_ms": e["median_ms"], "limit_ms": round(limit_de, 4), "holds": bool(e["median_ms"] <= limit_de)}}}
    for buf in (d_blob, d_off, d_idx, d_tiles, d_block, d_copy, d_back, d_st):
        buf.free()
    return out


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    tile_rows = int(argv[argv.index("--tile-rows") + 1]) if "--tile-rows" in argv else 90
    nt = tile_rows * TILES_ACROSS
    L, hip = lib(), _hip()
    ctx = gridfour_amd.GvrsHipContext(0)
    b = DeviceTileBatch(ctx, N_ROWS, N_COLS, nt, slot_stride=16)
    b.synth_dem(0x9E3779B97F4A7C15 + 2, TILES_ACROSS)
    ctx.synchronize()
    vals = b.get_values().reshape(nt, N_ROWS * N_COLS)
    b.free()
    timer = gridfour_amd.GpuTimer(ctx)
    out = {"workload": "etopo1: %d tile records of %dx%d cells, read as one block of %d x %d cells" % (nt, N_ROWS, N_COLS, tile_rows * N_ROWS,
                                                                                                     TILES_ACROSS * N_COLS),
           "codec_list": CODECS, "method": "HIP events, %d timings per case taken in turn in one process, checksums verified" % REPS,
           "csrc_digest": gridfour_amd.build.csrc_digest() if hasattr(gridfour_amd, "build") else None,
           "elements": [one_element(L, hip, ctx, timer, kind, vals, tile_rows) for kind in ("int", "short")]}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
