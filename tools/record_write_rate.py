"""What writing tile records on the device costs beside what the library could do before and beside what the read side pays for the
same checksums: the ETOPO1-shaped batch of tools/block_read_rate.py (12,960 tiles of 120 x 150 cells), codec list (CANON,),
checksums on.
    python tools/record_write_rate.py [--out profiles/record_write_rate.json] [--tile-rows 90]
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/record_write_rate.py --once
    python tools/record_write_rate.py --merge-kernel-stats <rocprofv3 kernel_stats.csv | results.db> <the JSON written above>
(--once: (a), (b), (c) and the verified decode once each, checked, and no timing loops: the run to put behind rocprofv3)
One process, the context's stream, HIP events, 20 timings per case taken in turn; medians with min and max:
  (a) gf_canon_encode_batch_i32_dev + gf_compact_dev: packings in one blob, no framing, no checksum (the record write replaces the compaction)
  (v) the read side's price of a checksum on the same records: gf_tile_record_decode_batch_dev with verification minus without
  (b) gf_tile_record_encode_batch_elems_dev, one INT element
  (c) gf_tile_record_encode_batch_elems_dev, two elements, short + int-coded float (reported only)
  (d) gf_tile_record_encode_batch, the host call, on the same tiles (wall clock, 3 calls; reported only)
The outputs are held against one another before anything is timed: (b)'s records equal (d)'s byte for byte, their packings are (a)'s,
and they read back.  Condition, reported as it comes out and asserted nowhere:  median(b) <= median(a) + (v) + spread(a)."""
import ctypes as C
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gridfour_amd  # noqa: E402
from gridfour_amd import DeviceBuffer, DeviceTileBatch, lib  # noqa: E402
from gridfour_amd._lib import check  # noqa: E402
from gridfour_amd.codec import _ELEM_SPEC  # noqa: E402

REPS = 20
CANON = 3
N_ROWS, N_COLS, TILES_ACROSS = 120, 150, 144


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "spread_ms": round(max(v) - min(v), 4), "reps": len(v)}


def _series(timer, fns):
    ms = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            timer.start()
            fn()
            timer.stop()
            ms[k].append(timer.elapsed_ms())
    return {k: _stats(v) for k, v in ms.items()}


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    once = "--once" in argv
    tile_rows = int(argv[argv.index("--tile-rows") + 1]) if "--tile-rows" in argv else 90
    nt, cells = tile_rows * TILES_ACROSS, N_ROWS * N_COLS
    L = lib()
    ctx = gridfour_amd.GvrsHipContext(0)
    tb = DeviceTileBatch(ctx, N_ROWS, N_COLS, nt, slot_stride=16)
    tb.synth_dem(0x9E3779B97F4A7C15 + 2, TILES_ACROSS)
    ctx.synchronize()
    vals = tb.get_values().reshape(nt, cells)
    tb.free()
    shorts = np.clip(vals, -32767, 32767).astype(np.int16)
    timer = gridfour_amd.GpuTimer(ctx)
    cd = (C.c_int * 1)(CANON)
    idx = np.arange(nt, dtype=np.int32)
    spec1 = np.zeros(1, _ELEM_SPEC)
    spec1["type"], spec1["scale"] = 0, 1.0
    spec2 = np.zeros(2, _ELEM_SPEC)
    spec2["type"], spec2["scale"], spec2["fill_i"] = [1, 3], [1.0, 10.0], [-32768, -9999]
    cap1 = nt * int(L.gf_tile_record_max_bytes_elems(_p(spec1), 1, N_ROWS, N_COLS))
    cap2 = nt * int(L.gf_tile_record_max_bytes_elems(_p(spec2), 2, N_ROWS, N_COLS))
    d_vals = DeviceBuffer(ctx, vals.nbytes + 16).upload(vals)
    d_shorts = DeviceBuffer(ctx, shorts.nbytes + 16).upload(shorts)
    d_idx = DeviceBuffer(ctx, nt * 4 + 16).upload(idx)
    stride = int(L.gf_huffman_default_stride(N_ROWS, N_COLS))
    d_slots = DeviceBuffer(ctx, nt * stride + 16)
    d_len = DeviceBuffer(ctx, nt * 4 + 16)
    d_est = DeviceBuffer(ctx, nt * 4 + 16)
    d_packs = DeviceBuffer(ctx, nt * stride + 16)
    d_poff = DeviceBuffer(ctx, (nt + 1) * 8 + 16)
    d_rec1 = DeviceBuffer(ctx, cap1 + 64)
    d_off1 = DeviceBuffer(ctx, (nt + 1) * 8 + 16)
    d_used = DeviceBuffer(ctx, 2 * nt + 16)
    d_st = DeviceBuffer(ctx, nt * 4 + 16)
    d_rec2 = DeviceBuffer(ctx, cap2 + 64)
    d_off2 = DeviceBuffer(ctx, (nt + 1) * 8 + 16)
    d_back = DeviceBuffer(ctx, vals.nbytes + 16)
    d_bidx = DeviceBuffer(ctx, nt * 4 + 16)
    p1 = (C.c_void_p * 1)(d_vals.ptr.value)
    p2 = (C.c_void_p * 2)(d_shorts.ptr.value, d_vals.ptr.value)

    def a_encode_compact():
        check(L.gf_canon_encode_batch_i32_dev(ctx.handle, None, 0, N_ROWS, N_COLS, nt, d_vals.ptr, d_slots.ptr, stride, d_len.ptr, None, d_est.ptr,
                                              0xF), "gf_canon_encode_batch_i32_dev")
        check(L.gf_compact_dev(ctx.handle, None, nt, d_slots.ptr, stride, d_len.ptr, d_poff.ptr, d_packs.ptr, nt * stride), "gf_compact_dev")

    def b_records_one():
        check(L.gf_tile_record_encode_batch_elems_dev(ctx.handle, None, cd, 1, _p(spec1), 1, N_ROWS, N_COLS, nt, d_idx.ptr, p1, 1, d_rec1.ptr,
                                                      cap1, d_off1.ptr, d_used.ptr, d_st.ptr), "gf_tile_record_encode_batch_elems_dev")

    def c_records_two():
        check(L.gf_tile_record_encode_batch_elems_dev(ctx.handle, None, cd, 1, _p(spec2), 2, N_ROWS, N_COLS, nt, d_idx.ptr, p2, 1, d_rec2.ptr,
                                                      cap2, d_off2.ptr, d_used.ptr, d_st.ptr), "gf_tile_record_encode_batch_elems_dev")

    # every case once outside the timings (buffers grow, code objects load); the outputs against one another
    a_encode_compact()
    b_records_one()
    ctx.synchronize()
    assert (d_st.download(np.int32, nt) == 0).all() and (d_est.download(np.int32, nt) == 0).all()
    off1 = d_off1.download(np.uint64, nt + 1)
    total1 = int(off1[nt])
    rec1 = d_rec1.download(np.uint8, total1)
    poff = d_poff.download(np.uint64, nt + 1)
    packs = d_packs.download(np.uint8, int(poff[nt]))
    used1 = d_used.download(np.uint8, nt)
    for t in range(0, nt, 97):                                              # (b)'s element bytes are (a)'s packings
        n = int(poff[t + 1] - poff[t])
        r = rec1[int(off1[t]):int(off1[t + 1])]
        assert used1[t] == 0 and int(r[12:16].view("<u4")[0]) == n and np.array_equal(r[16:16 + n], packs[int(poff[t]):int(poff[t + 1])]), t
    h_blob = np.empty(cap1, np.uint8)
    h_off = np.zeros(nt + 1, np.uint64)
    h_used = np.zeros(nt, np.uint8)

    def d_host():
        check(L.gf_tile_record_encode_batch(ctx.handle, cd, 1, 0, 0, N_ROWS, N_COLS, nt, _p(idx), _p(vals), 1, _p(h_blob), cap1, _p(h_off),
                                            _p(h_used)), "gf_tile_record_encode_batch")

    sums = {"b_records": zlib.crc32(rec1.tobytes())}
    if not once:
        d_host()
        assert np.array_equal(h_off, off1) and np.array_equal(h_used, used1)
        sums["d_host_records"] = zlib.crc32(h_blob[:total1].tobytes())
        assert sums["b_records"] == sums["d_host_records"], sums

    def v_decode(verify):
        def run():
            check(L.gf_tile_record_decode_batch_dev(ctx.handle, None, cd, 1, 0, N_ROWS, N_COLS, nt, d_rec1.ptr, total1, d_off1.ptr, verify,
                                                    d_bidx.ptr, d_back.ptr, d_st.ptr), "gf_tile_record_decode_batch_dev")
        return run

    v_decode(1)()
    ctx.synchronize()
    assert (d_st.download(np.int32, nt) == 0).all() and np.array_equal(d_bidx.download(np.int32, nt), idx)
    assert np.array_equal(d_back.download(np.int32, nt * cells).reshape(nt, cells), vals)
    c_records_two()
    ctx.synchronize()
    assert (d_st.download(np.int32, nt) == 0).all()
    total2 = int(d_off2.download(np.uint64, nt + 1)[nt])
    used2 = d_used.download(np.uint8, 2 * nt)
    if once:
        print("once: %d tiles, %d record bytes (one int), %d (short + icf)" % (nt, total1, total2))
        return

    r = _series(timer, {"a_canon_encode_plus_compact": a_encode_compact, "v_decode_verify": v_decode(1), "v_decode_no_verify": v_decode(0),
                        "b_records_one_int": b_records_one, "c_records_short_icf": c_records_two})
    ctx.synchronize()
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        d_host()
        wall.append((time.perf_counter() - t0) * 1e3)
    r["d_host_tile_record_encode_batch_wall"] = _stats(wall)
    a, b = r["a_canon_encode_plus_compact"], r["b_records_one_int"]
    v = round(r["v_decode_verify"]["median_ms"] - r["v_decode_no_verify"]["median_ms"], 4)
    limit = round(a["median_ms"] + v + a["spread_ms"], 4)
    for k in ("a_canon_encode_plus_compact", "b_records_one_int", "d_host_tile_record_encode_batch_wall"):
        r[k]["GBps_of_cells"] = round(vals.nbytes / 1e9 / (r[k]["median_ms"] / 1e3), 1)
    r["c_records_short_icf"]["GBps_of_cells"] = round((vals.nbytes + shorts.nbytes) / 1e9 / (r["c_records_short_icf"]["median_ms"] / 1e3), 1)
    out = {"workload": "etopo1: %d tiles of %dx%d cells, codec list (CANON,), checksums on" % (nt, N_ROWS, N_COLS),
           "method": "HIP events on the context's stream, %d timings per case taken in turn in one process; (d) wall clock, 3 calls" % REPS,
           "csrc_digest": gridfour_amd.build.csrc_digest() if hasattr(gridfour_amd, "build") else None,
           "record_bytes_one_int": total1, "record_bytes_short_icf": total2, "packing_bytes": int(poff[nt]),
           "winners_one_int": {int(x): int(n) for x, n in zip(*np.unique(used1, return_counts=True))},
           "winners_short_icf": {int(x): int(n) for x, n in zip(*np.unique(used2, return_counts=True))},
           "output_crc32": sums, "cases": r, "v_checksum_price_ms": v,
           "condition": {"b_le_a_plus_v_plus_spread_a": {"value_ms": b["median_ms"], "limit_ms": limit,
                                                         "verdict": "holds" if b["median_ms"] <= limit else "DOES NOT HOLD"}}}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


def merge_kernel_stats(stats_path, json_path):
    """per-kernel times from one `rocprofv3 --kernel-trace --stats` run of --once into the JSON written by the timing run: the
    run's kernel_stats.csv, or its rocpd database (results.db, where rocprofv3 writes no CSV by default)"""
    with open(json_path) as f:
        out = json.load(f)
    if stats_path.endswith(".db"):
        import sqlite3
        db = sqlite3.connect(stats_path)
        table = [(n, c, a, lo, hi) for n, c, a, lo, hi in db.execute(
            "select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels group by name")]
    else:
        import csv
        with open(stats_path, newline="") as f:
            table = [(r.get("Name", ""), int(r["Calls"]), float(r["AverageNs"]), float(r["MinNs"]), float(r["MaxNs"])) for r in csv.DictReader(f)]
    rows = {}
    for name, calls, avg, lo, hi in table:
        k = next((w for w in name.replace("(", " ").replace("<", " ").replace(":", " ").split() if w.startswith("k_")), name)
        rows[k if k not in rows else name] = {"calls": int(calls), "average_us": round(avg / 1e3, 2), "min_us": round(lo / 1e3, 2),
                                              "max_us": round(hi / 1e3, 2)}
    out["kernels_once"] = dict(sorted(rows.items()))
    with open(json_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["kernels_once"], indent=1))


if __name__ == "__main__":
    if "--merge-kernel-stats" in sys.argv:
        i = sys.argv.index("--merge-kernel-stats")
        merge_kernel_stats(sys.argv[i + 1], sys.argv[i + 2])
    else:
        main(sys.argv[1:])
