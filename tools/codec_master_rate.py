"""Throughput of the default-codec-list path: what CodecMaster.encode (gvrs/CodecMaster.java:142-193) and
RecordManager.writeTile (gvrs/RecordManager.java:386-490) would call with the standard codec list Huffman / Deflate / Float /
CanonHuffman... of GvrsFileSpecification.java:221-230 -- gf_codec_master_{encode,decode}_batch_i32 and
gf_tile_record_{encode,decode}_batch on an ETOPO1-shaped batch in host memory; next to it the rate of the host's zlib alone on
the M32 streams the Deflate candidates consist of (the bound of anything that must reproduce zlib's bytes).
    python tools/codec_master_rate.py [nTiles] [codec list, e.g. 1,2,0,3]
Device-records mode: the same batch as tile records (gf_tile_record_encode_batch), decoded where they lie in device memory by
gf_tile_record_decode_batch_dev -- HIP events on one stream, with and without checksum verification, with and without the one
H2D copy of the blob (from page-locked memory) -- beside the host call gf_tile_record_decode_batch in the same run:
    python tools/codec_master_rate.py --device-records [nTiles] [codec list] [--once] [--out profiles/device_records_rate.json]
                                      [--elements short,float] [--parent-lib <libgvrs_hip.so of the parent commit>]
    python tools/codec_master_rate.py --merge-kernel-stats <rocprofv3 kernel_stats.csv> <the JSON written above>
(--once: one call of each form and no timing loops, the run to put behind `rocprofv3 --kernel-trace --stats --`)
--elements LIST (int, short, float, icf; e.g. short,float) adds gf_tile_record_decode_batch_elems_dev to the same run, checksums
verified, medians of 20 event timings with the calls taken in turn: (1) gf_tile_record_decode_batch_dev on the int records, the
baseline, (2) the new call on the same records as one INT element -- the gate: its median within the spread (max - min) that (1)
shows in this run --, (3) the new call on records of the listed elements, framed here from the existing encoders' packings
(reported, not gated).
--parent-lib PATH runs this alone: gf_tile_record_decode_batch_dev of the library at PATH (a build of the parent commit; the C ABI
is the same) and of this tree's, in one process on one stream, checksums verified, 20 event timings each taken in turn, on (int)
the batch's INT records, every record on one codec: the straight route, (short) the batch as SHORT records: every tile decoded to
the temporary and narrowed, (half_standard) INT records with every second record left in standard form: half the tiles copied
from the temporary, half from the blob.  The gate per case: this tree's median <= the parent's median + the parent's own spread.
With --out the result replaces the key "parent_vs_unified" of that file and nothing else."""
import ctypes as C
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gridfour_amd  # noqa: E402
from gridfour_amd import DeviceTileBatch, lib  # noqa: E402
from gridfour_amd._lib import check  # noqa: E402


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def main():
    nt = int(sys.argv[1]) if len(sys.argv) > 1 else 12960
    codecs = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "1,2,0,3").split(",")]
    n_rows, n_cols = 120, 150
    cells = n_rows * n_cols
    ctx = gridfour_amd.GvrsHipContext(0)
    b = DeviceTileBatch(ctx, n_rows, n_cols, nt, slot_stride=16)
    b.synth_dem(0x9E3779B97F4A7C15 + 2, 144)
    ctx.synchronize()
    vals = b.get_values().reshape(nt, cells)
    del b
    L = lib()
    cd = (C.c_int * len(codecs))(*codecs)
    gb = vals.nbytes / 1e9
    out = {"workload": "etopo1: %d tiles of %dx%d int32 (%.2f GB) in pageable host memory" % (nt, n_rows, n_cols, gb), "codec_list": codecs,
           "threads": len(os.sched_getaffinity(0))}

    cap = nt * (cells + 4096)
    blob = np.empty(cap, np.uint8)
    off = np.zeros(nt + 1, np.uint64)
    used = np.zeros(nt, np.uint8)
    st = np.zeros(nt, np.int32)

    def timed(fn, reps=2):
        best = 1e30
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            best = min(best, time.perf_counter() - t0)
        return best

    t = timed(lambda: check(L.gf_codec_master_encode_batch_i32(ctx.handle, cd, len(codecs), n_rows, n_cols, nt, _p(vals), _p(blob), cap,
                                                               _p(off), _p(used), _p(st)), "codec_master_encode"))
    total = int(off[nt])
    u, c = np.unique(used, return_counts=True)
    out["codec_master_encode"] = {"seconds": round(t, 4), "GBps": round(gb / t, 3), "bytes_per_cell": round(total / (nt * cells), 4),
                                  "winners": {int(a): int(n) for a, n in zip(u, c)}}
    back = np.empty_like(vals)
    t = timed(lambda: check(L.gf_codec_master_decode_batch_i32(ctx.handle, cd, len(codecs), n_rows, n_cols, nt, _p(blob), _p(off), _p(back),
                                                               _p(st)), "codec_master_decode"))
    assert (st == 0).all() and np.array_equal(back, vals)
    out["codec_master_decode"] = {"seconds": round(t, 4), "GBps": round(gb / t, 3)}

    # tile records (RecordManager.writeTile framing)
    rcap = nt * int(L.gf_tile_record_max_bytes(0, n_rows, n_cols))
    rblob = np.empty(rcap, np.uint8)
    roff = np.zeros(nt + 1, np.uint64)
    idx = np.arange(nt, dtype=np.int32)
    t = timed(lambda: check(L.gf_tile_record_encode_batch(ctx.handle, cd, len(codecs), 0, -2 ** 31, n_rows, n_cols, nt, _p(idx), _p(vals), 1,
                                                          _p(rblob), rcap, _p(roff), _p(used)), "tile_record_encode"))
    out["tile_record_encode"] = {"seconds": round(t, 4), "GBps": round(gb / t, 3), "record_bytes_per_cell": round(int(roff[nt]) / (nt * cells), 4)}
    ridx = np.zeros(nt, np.int32)
    t = timed(lambda: check(L.gf_tile_record_decode_batch(ctx.handle, cd, len(codecs), 0, n_rows, n_cols, nt, _p(rblob), _p(roff), 1, _p(ridx),
                                                          _p(back), _p(st)), "tile_record_decode"))
    assert (st == 0).all() and np.array_equal(back, vals) and np.array_equal(ridx, idx)
    out["tile_record_decode"] = {"seconds": round(t, 4), "GBps": round(gb / t, 3)}

    # the single codecs through their host entry points (what the list is made of)
    for name in ("huffman", "canon", "deflate"):
        fn = getattr(L, "gf_%s_encode_batch_i32" % name)
        t = timed(lambda: check(fn(ctx.handle, 0, n_rows, n_cols, nt, _p(vals), _p(blob), cap, _p(off), _p(used), _p(st)), name))
        out["%s_encode_host_path" % name] = {"seconds": round(t, 4), "GBps": round(gb / t, 3), "bytes_per_cell": round(int(off[nt]) / (nt * cells), 4)}

    # the bound: zlib level 6 alone on the M32 streams of the Deflate candidates (three per tile without nulls), all threads
    import oracle
    sample = min(nt, 256)
    streams = []
    for ti in range(sample):
        for p in (1, 2, 3):
            streams.append(bytes(oracle.predictor_encode(p, n_rows, n_cols, vals[ti])[0]))
    nthreads = len(os.sched_getaffinity(0))

    def work(chunk):
        return sum(len(zlib.compress(s, 6)) for s in chunk)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(nthreads) as ex:
        list(ex.map(work, [streams[i::nthreads] for i in range(nthreads)]))
    tz = time.perf_counter() - t0
    t0 = time.perf_counter()
    work(streams[:48])
    t1 = time.perf_counter() - t0
    m32_bytes = sum(map(len, streams))
    out["zlib_alone"] = {"sample_tiles": sample, "m32_bytes_per_tile": round(m32_bytes / sample), "level": 6,
                         "one_thread_MBps_of_m32": round(sum(map(len, streams[:48])) / t1 / 1e6, 1),
                         "all_threads_MBps_of_m32": round(m32_bytes / tz / 1e6, 1),
                         "bound_GBps_of_cells": round(sample * cells * 4 / tz / 1e9, 3),
                         "note": "three candidate streams per tile (CodecDeflate.java:176-199) deflated by zlib level 6 on every thread "
                                 "of the box: no implementation that reproduces zlib's bytes encodes the list faster than this"}
    print(json.dumps(out))


RECORD_KERNELS = ("k_codec_partition", "k_record_parse_elems", "k_record_crc32c_elems", "k_elem_scatter")
ELEM_TYPES = {"int": 0, "short": 1, "float": 2, "icf": 3}


def _frame_records(L, elements):
    """[record][element] bytes -> (blob, offsets) of RecordManager's framing with CRC-32C, tile index = record number"""
    import struct
    recs = []
    for i, els in enumerate(elements):
        body = b"".join(struct.pack("<i", len(el)) + el for el in els)
        size = (4 + len(body) + 12 + 7) // 8 * 8
        r = bytearray(size)
        struct.pack_into("<iB3xi", r, 0, size, 2, i)
        r[12:12 + len(body)] = body
        struct.pack_into("<I", r, size - 4, L.gf_crc32c(C.c_char_p(bytes(r[:size - 4])), size - 4))
        recs.append(bytes(r))
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    return np.frombuffer(b"".join(recs) + b"\0" * 64, np.uint8), off


def _series(timer, fns, reps):
    """event timings of several calls taken in turn, reps of each: median, extremes and the spread a call shows against itself"""
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            timer.start()
            fn()
            timer.stop()
            ms[k].append(timer.elapsed_ms())
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "spread_ms": round(max(v) - min(v), 4), "reps": reps} for k, v in ms.items()}


def _elements_run(L, ctx, timer, cd, codecs, names, n_rows, n_cols, vals, old_call, d_blob, total, d_off, d_idx, d_val, d_st, once):
    from gridfour_amd.codec import _ELEM_SPEC
    nt, cells = vals.shape
    idx = np.arange(nt, dtype=np.int32)
    reps = 1 if once else 20
    # (2) the int records of the baseline as ONE INT element
    spec1 = np.zeros(1, _ELEM_SPEC)
    spec1["scale"] = 1.0
    ptr1 = (C.c_void_p * 1)(d_val.ptr.value)

    def one_element():
        check(L.gf_tile_record_decode_batch_elems_dev(ctx.handle, None, cd, len(codecs), _p(spec1), 1, n_rows, n_cols, nt, d_blob.ptr, total,
                                                      d_off.ptr, 1, d_idx.ptr, ptr1, d_st.ptr), "gf_tile_record_decode_batch_elems_dev")
    d_val.fill(0)
    one_element()
    ctx.synchronize()
    assert (d_st.download(np.int32, nt) == 0).all() and np.array_equal(d_idx.download(np.int32, nt), idx)
    assert np.array_equal(d_val.download(np.int32, nt * cells).reshape(nt, cells), vals)
    # (3) records of the listed elements: int-coded elements hold the batch's cells (shorts clipped), float elements a tenth of them
    shorts = np.clip(vals, -32767, 32767).astype(np.int32)
    floats = (vals.astype(np.float32) * np.float32(0.1)).astype(np.float32)
    src = {"int": vals, "icf": vals, "short": shorts, "float": floats}
    cap = nt * (5 * cells + 4096)
    packs = {}
    for kind in set(names):
        blob = np.empty(cap, np.uint8)
        off = np.zeros(nt + 1, np.uint64)
        if kind == "float":
            check(L.gf_float_encode_batch_f32(ctx.handle, codecs.index(0), n_rows, n_cols, nt, _p(floats), 6, _p(blob), cap, _p(off)), "float_encode")
        else:
            used, st = np.zeros(nt, np.uint8), np.zeros(nt, np.int32)
            check(L.gf_codec_master_encode_batch_i32(ctx.handle, cd, len(codecs), n_rows, n_cols, nt, _p(src[kind]), _p(blob), cap, _p(off), _p(used),
                                                     _p(st)), "codec_master_encode")
            assert (st == 0).all()
        packs[kind] = (blob, off)
    std = {"int": src["int"].astype("<i4"), "icf": src["icf"].astype("<i4"), "short": shorts.astype("<i2"), "float": floats.astype("<f4")}
    elements = []
    for t in range(nt):
        els = []
        for kind in names:
            blob, off = packs[kind]
            pk = bytes(blob[int(off[t]):int(off[t + 1])])
            raw = std[kind][t].tobytes()
            els.append(pk if len(pk) < len(raw) else raw)                 # (120 x 150 cells: the short form needs no padding)
        elements.append(els)
    eblob, eoff = _frame_records(L, elements)
    etotal = int(eoff[nt])
    specs = np.zeros(len(names), _ELEM_SPEC)
    specs["type"] = [ELEM_TYPES[k] for k in names]
    specs["scale"], specs["fill_i"], specs["fill_f"] = 1.0, -2 ** 31, np.nan
    dtypes = [{"int": np.int32, "short": np.int16}.get(k, np.float32) for k in names]
    e_blob = gridfour_amd.DeviceBuffer(ctx, etotal + 64).upload(eblob[:etotal + 64])
    e_off = gridfour_amd.DeviceBuffer(ctx, eoff.nbytes).upload(eoff)
    e_val = [gridfour_amd.DeviceBuffer(ctx, nt * cells * np.dtype(dt).itemsize).fill(0) for dt in dtypes]
    e_st = gridfour_amd.DeviceBuffer(ctx, len(names) * nt * 4)
    ptrs = (C.c_void_p * len(names))(*[b.ptr.value for b in e_val])

    def listed_elements():
        check(L.gf_tile_record_decode_batch_elems_dev(ctx.handle, None, cd, len(codecs), _p(specs), len(names), n_rows, n_cols, nt, e_blob.ptr,
                                                      etotal, e_off.ptr, 1, d_idx.ptr, ptrs, e_st.ptr), "gf_tile_record_decode_batch_elems_dev")
    listed_elements()
    ctx.synchronize()
    assert (e_st.download(np.int32, len(names) * nt) == 0).all() and np.array_equal(d_idx.download(np.int32, nt), idx)
    for k, b, dt in zip(names, e_val, dtypes):
        got = b.download(dt, nt * cells).reshape(nt, cells)
        want = src[k].astype(np.float32) if k == "icf" else src[k].astype(dt)
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), k
    res = _series(timer, {"old_call": old_call, "new_call_one_element": one_element, "new_call_elements": listed_elements}, reps)
    gb = vals.nbytes / 1e9
    res["old_call"]["GBps_of_cells"] = round(gb / (res["old_call"]["median_ms"] / 1e3), 2)
    res["new_call_one_element"]["GBps_of_cells"] = round(gb / (res["new_call_one_element"]["median_ms"] / 1e3), 2)
    cell_bytes = sum(nt * cells * np.dtype(dt).itemsize for dt in dtypes)
    res["new_call_elements"].update({"elements": list(names), "record_bytes": etotal, "cell_bytes": cell_bytes,
                                     "GBps_of_cells": round(cell_bytes / 1e9 / (res["new_call_elements"]["median_ms"] / 1e3), 2)})
    gap = res["new_call_one_element"]["median_ms"] - res["old_call"]["median_ms"]
    res["one_element_gap_ms"] = round(gap, 4)
    res["one_element_within_old_spread"] = bool(abs(gap) <= res["old_call"]["spread_ms"])
    for b in [e_blob, e_off, e_st] + e_val:
        b.free()
    return res


def _parent_vs_unified(L, ctx, timer, parent_path, cd, codecs, n_rows, n_cols, vals, int_records, once):
    from gridfour_amd._lib import SIGNATURES
    nt, cells = vals.shape
    P = C.CDLL(parent_path)
    for name in ("gf_context_create", "gf_context_destroy", "gf_tile_record_decode_batch_dev"):
        getattr(P, name).restype, getattr(P, name).argtypes = SIGNATURES[name]
    pctx = C.c_void_p()
    check(P.gf_context_create(0, C.byref(pctx)), "gf_context_create (parent)")
    stream = ctx.stream                                  # both builds run on this context's stream, where the timer's events are
    assert stream
    idx = np.arange(nt, dtype=np.int32)
    shorts = np.clip(vals, -32767, 32767).astype(np.int32)

    def packings(values):
        cap = nt * (4 * cells + 1024) + 64
        blob, off = np.empty(cap, np.uint8), np.zeros(nt + 1, np.uint64)
        used, st = np.zeros(nt, np.uint8), np.zeros(nt, np.int32)
        check(L.gf_codec_master_encode_batch_i32(ctx.handle, cd, len(codecs), n_rows, n_cols, nt, _p(values), _p(blob), cap, _p(off), _p(used),
                                                 _p(st)), "codec_master_encode")
        assert (st == 0).all()
        return [bytes(blob[int(off[t]):int(off[t + 1])]) for t in range(nt)]

    def framed(elements):
        blob, off = _frame_records(L, [[el] for el in elements])
        total = int(off[nt])
        return gridfour_amd.DeviceBuffer(ctx, total + 64).upload(blob[:total + 64]), total, gridfour_amd.DeviceBuffer(ctx, off.nbytes).upload(off)

    raw2 = shorts.astype("<i2")
    raw4 = vals.astype("<i4")
    cases = {"int": (0, vals, int_records),
             "short": (1, shorts.astype(np.int16), framed([pk if len(pk) < 2 * cells else raw2[t].tobytes() for t, pk in enumerate(packings(shorts))])),
             "half_standard": (0, vals, framed([pk if t % 2 == 0 and len(pk) < 4 * cells else raw4[t].tobytes() for t, pk in enumerate(packings(vals))]))}
    d_idx = gridfour_amd.DeviceBuffer(ctx, nt * 4)
    d_val = gridfour_amd.DeviceBuffer(ctx, nt * cells * 4)
    d_st = gridfour_amd.DeviceBuffer(ctx, nt * 4)
    res = {}
    for name, (elem, want, (d_blob, total, d_off)) in cases.items():
        def call(lib, handle):
            check(lib.gf_tile_record_decode_batch_dev(handle, stream, cd, len(codecs), elem, n_rows, n_cols, nt, d_blob.ptr, total, d_off.ptr, 1,
                                                      d_idx.ptr, d_val.ptr, d_st.ptr), "gf_tile_record_decode_batch_dev")
        fns = {"parent": lambda: call(P, pctx), "unified": lambda: call(L, ctx.handle)}
        for fn in fns.values():                           # (grows the contexts' buffers, and the answer is checked once per build)
            d_val.fill(0)
            d_st.fill(0xff)
            fn()
            ctx.synchronize()
            assert (d_st.download(np.int32, nt) == 0).all() and np.array_equal(d_idx.download(np.int32, nt), idx)
            assert np.array_equal(d_val.download(want.dtype, nt * cells).reshape(nt, cells), want), name
        r = _series(timer, fns, 1 if once else 20)
        r["record_bytes"] = total
        r["gap_ms"] = round(r["unified"]["median_ms"] - r["parent"]["median_ms"], 4)
        r["unified_within_parent_spread"] = bool(r["unified"]["median_ms"] <= r["parent"]["median_ms"] + r["parent"]["spread_ms"])
        res[name] = r
    P.gf_context_destroy(pctx)
    return res


def device_records(argv):
    once = "--once" in argv
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    names = argv[argv.index("--elements") + 1].split(",") if "--elements" in argv else None
    assert names is None or (names and all(k in ELEM_TYPES for k in names)), names
    parent = argv[argv.index("--parent-lib") + 1] if "--parent-lib" in argv else None
    pos = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in ("--out", "--elements", "--parent-lib"))]
    nt = int(pos[0]) if pos else 12960
    codecs = [int(x) for x in (pos[1] if len(pos) > 1 else "1,2,0,3").split(",")]
    n_rows, n_cols = 120, 150
    cells = n_rows * n_cols
    ctx = gridfour_amd.GvrsHipContext(0)
    b = DeviceTileBatch(ctx, n_rows, n_cols, nt, slot_stride=16)
    b.synth_dem(0x9E3779B97F4A7C15 + 2, 144)
    ctx.synchronize()
    vals = b.get_values().reshape(nt, cells)
    del b
    L = lib()
    cd = (C.c_int * len(codecs))(*codecs)
    gb = vals.nbytes / 1e9
    rcap = nt * int(L.gf_tile_record_max_bytes(0, n_rows, n_cols))
    rblob = np.empty(rcap, np.uint8)
    roff = np.zeros(nt + 1, np.uint64)
    idx = np.arange(nt, dtype=np.int32)
    used = np.zeros(nt, np.uint8)
    check(L.gf_tile_record_encode_batch(ctx.handle, cd, len(codecs), 0, -2 ** 31, n_rows, n_cols, nt, _p(idx), _p(vals), 1, _p(rblob), rcap,
                                        _p(roff), _p(used)), "tile_record_encode")
    total = int(roff[nt])
    u, c = np.unique(used, return_counts=True)
    out = {"workload": "etopo1: %d tile records of %dx%d int32 (%.2f GB of cells, %.3f GB of records)" % (nt, n_rows, n_cols, gb, total / 1e9),
           "codec_list": codecs, "winners": {int(a): int(n) for a, n in zip(u, c)}, "threads": len(os.sched_getaffinity(0))}
    # the records in page-locked memory (a reader's file buffer), and the device side
    pinned = C.c_void_p()
    check(L.gf_host_alloc(total + 64, C.byref(pinned)), "gf_host_alloc")
    C.memmove(pinned, _p(rblob), total)
    d_blob = gridfour_amd.DeviceBuffer(ctx, total + 64)
    d_off = gridfour_amd.DeviceBuffer(ctx, roff.nbytes).upload(roff)
    d_idx = gridfour_amd.DeviceBuffer(ctx, nt * 4)
    d_val = gridfour_amd.DeviceBuffer(ctx, nt * cells * 4)
    d_st = gridfour_amd.DeviceBuffer(ctx, nt * 4)
    timer = gridfour_amd.GpuTimer(ctx)

    def upload():
        check(L.gf_dev_upload(ctx.handle, d_blob.ptr, pinned, total), "gf_dev_upload")

    def decode(verify):
        check(L.gf_tile_record_decode_batch_dev(ctx.handle, None, cd, len(codecs), 0, n_rows, n_cols, nt, d_blob.ptr, total, d_off.ptr, verify,
                                                d_idx.ptr, d_val.ptr, d_st.ptr), "gf_tile_record_decode_batch_dev")

    def measure(fn, reps):
        ms, wall = 1e30, 1e30
        for _ in range(reps):
            t0 = time.perf_counter()
            timer.start()
            fn()
            timer.stop()
            ms = min(ms, timer.elapsed_ms())
            wall = min(wall, time.perf_counter() - t0)
        return {"event_ms": round(ms, 4), "wall_seconds": round(wall, 5), "GBps_of_cells": round(gb / (ms / 1e3), 2)}

    back = np.empty_like(vals)
    ridx = np.zeros(nt, np.int32)
    st = np.zeros(nt, np.int32)

    def host():
        check(L.gf_tile_record_decode_batch(ctx.handle, cd, len(codecs), 0, n_rows, n_cols, nt, _p(rblob), _p(roff), 1, _p(ridx), _p(back),
                                            _p(st)), "tile_record_decode")

    upload()
    decode(1)                                             # (grows the context's buffers: not part of any timing)
    ctx.synchronize()
    assert (d_st.download(np.int32, nt) == 0).all() and np.array_equal(d_idx.download(np.int32, nt), idx)
    assert np.array_equal(d_val.download(np.int32, nt * cells).reshape(nt, cells), vals)
    if parent:
        res = _parent_vs_unified(L, ctx, timer, parent, cd, codecs, n_rows, n_cols, vals, (d_blob, total, d_off), once)
        print(json.dumps({"workload": out["workload"], "parent_vs_unified": res}))
        if out_path and not once:
            with open(out_path) as f:
                merged = json.load(f)
            merged["parent_vs_unified"] = res
            with open(out_path, "w") as f:
                json.dump(merged, f, indent=1)
                f.write("\n")
        L.gf_host_free(pinned)
        return
    reps = 1 if once else 5
    out["device_verify"] = measure(lambda: decode(1), reps)
    out["device_no_verify"] = measure(lambda: decode(0), reps)
    out["device_verify_with_h2d"] = measure(lambda: (upload(), decode(1)), reps)
    out["device_no_verify_with_h2d"] = measure(lambda: (upload(), decode(0)), reps)
    host()                                                # (warm: staging buffers of the host pipeline)
    t = 1e30
    for _ in range(1 if once else 3):
        t0 = time.perf_counter()
        host()
        t = min(t, time.perf_counter() - t0)
    assert (st == 0).all() and np.array_equal(back, vals) and np.array_equal(ridx, idx)
    out["host_call_verify"] = {"wall_seconds": round(t, 5), "GBps_of_cells": round(gb / t, 2),
                               "note": "gf_tile_record_decode_batch: bytes and cells in pageable host memory, the D2H copy of the cells included"}
    out["device_with_h2d_not_slower_than_host"] = bool(out["device_verify_with_h2d"]["wall_seconds"] <= t)
    if names:
        upload()
        out["elems"] = _elements_run(L, ctx, timer, cd, codecs, names, n_rows, n_cols, vals, lambda: decode(1), d_blob, total, d_off, d_idx, d_val,
                                     d_st, once)
    L.gf_host_free(pinned)
    text = json.dumps(out)
    print(text)
    if out_path and not once:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def merge_kernel_stats(csv_path, json_path):
    """per-kernel times of the record kernels from one `rocprofv3 --kernel-trace --stats` run into the JSON of the mode above"""
    import csv
    with open(json_path) as f:
        out = json.load(f)
    rows = {}
    with open(csv_path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            hits = [k for k in RECORD_KERNELS if k in name]
            if hits:
                assert len(hits) == 1, (name, hits)                      # (no name in RECORD_KERNELS may be part of another)
                k = hits[0]
                rows[k] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                           "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    out["kernels"] = rows
    with open(json_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(rows))


if __name__ == "__main__":
    if "--merge-kernel-stats" in sys.argv:
        i = sys.argv.index("--merge-kernel-stats")
        merge_kernel_stats(sys.argv[i + 1], sys.argv[i + 2])
    elif "--device-records" in sys.argv:
        device_records([a for a in sys.argv[1:] if a != "--device-records"])
    else:
        main()
