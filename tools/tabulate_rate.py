"""What tabulating a device-resident block costs: the ETOPO1-shaped block, 10,800 x 21,600 cells from gf_synth_dem_dev.
    python tools/tabulate_rate.py [--out profiles/tabulate_rate.json] [--shrink K]
HIP events on the context's stream, warm-up, then 20 (dense) / 7 (symbols) timings per case taken in turn in one process; medians,
min and max.  Before the timings every dense result is compared bit for bit with the CPU harness (tests/csrc/tabulate_harness.cpp),
the INT symbol table with numpy's count of the same raster, and both symbol forms with the numpy model on the raster's first rows.
  dense_short_ref / dense_int_ref   gf_block_tabulate_dense_dev with the reference's window -11000 .. 8650 at scale 1 (19,652
                     counters: private to the workgroup in LDS)
  dense_int_global   the same block with a window beyond GF_TAB_LDS_MAX_BINS counters: global atomics
  copy_d2d_*         a device-to-device copy of the same block's bytes: the memory yardstick (it reads AND writes them)
  host_*             the host loop a caller had before: the stand-alone C++ harness (g++ -O2 -ffp-contract=off) on 16 threads over
                     the block in host memory; wall clock, 3 timings, the download of the block not counted
  symbols_int / symbols_float   gf_block_tabulate_symbols_dev; the FLOAT block is the INT block plus a fractional part, so that
                     most symbols are distinct
  rocprim_sort_*     rocprim::radix_sort_keys on the same keys (tools/csrc/tab_rocprim_sort.hip, compiled into the tool only): the
                     tabulation does that sort's work plus one pass over the keys for the runs
No threshold is set: the numbers are written as they come out.  --shrink K divides both sides of the block by K (a quick look)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gridfour_amd  # noqa: E402
from gridfour_amd import DeviceBuffer, DeviceTileBatch, lib  # noqa: E402
from gridfour_amd import build as hipbuild  # noqa: E402
from gridfour_amd._lib import check  # noqa: E402
from gridfour_amd.codec import TAB_SUMMARY, TAB_SYMBOLS  # noqa: E402
import tabulate_cases as K  # noqa: E402
import tabulate_ref as R  # noqa: E402

REPS, SYM_REPS, HOST_REPS, HOST_THREADS = 20, 7, 3, 16
N_ROWS, N_COLS, TILES_ACROSS, TILE_ROWS = 120, 150, 144, 90
GLOBAL_RANGE = (-11000, 8650 + 20000, 1.0)


def _hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("libamdhip64 not loadable")


def build_yardstick():
    src, so = os.path.join(ROOT, "tools", "csrc", "tab_rocprim_sort.hip"), os.path.join(ROOT, "tools", "bin", "libtab_rocprim.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call([hipbuild._hipcc(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    Y = C.CDLL(so)
    Y.tr_sort_temp_bytes.argtypes = [C.c_size_t, C.POINTER(C.c_size_t)]
    Y.tr_sort.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return Y


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v)}


def _timed(timer, cases, reps):
    for fn in cases.values():                                              # warm-up: every case once outside the timings
        fn()
    ms = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            timer.start()
            fn()
            timer.stop()
            ms[k].append(timer.elapsed_ms())
    return {k: _stats(v) for k, v in ms.items()}


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    shrink = int(argv[argv.index("--shrink") + 1]) if "--shrink" in argv else 1
    tile_rows, tiles_across = max(TILE_ROWS // shrink, 1), max(TILES_ACROSS // shrink, 1)
    nt = tile_rows * tiles_across
    if "--build-only" in argv:
        build_yardstick()
        K.build_harness()
        return
    L, hip, Y, th = lib(), _hip(), build_yardstick(), K.build_harness()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    ctx = gridfour_amd.GvrsHipContext(0)
    timer = gridfour_amd.GpuTimer(ctx)
    stream = C.c_void_p(ctx.stream)
    b = DeviceTileBatch(ctx, N_ROWS, N_COLS, nt, slot_stride=16)
    b.synth_dem(0x9E3779B97F4A7C15 + 2, tiles_across)
    ctx.synchronize()
    vals = b.get_values().reshape(nt, N_ROWS * N_COLS)
    b.free()
    rows, cols = tile_rows * N_ROWS, tiles_across * N_COLS
    n = rows * cols
    raster_i = np.ascontiguousarray(vals.reshape(tile_rows, tiles_across, N_ROWS, N_COLS).transpose(0, 2, 1, 3).reshape(n))
    del vals
    raster_s = np.clip(raster_i, -32767, 32767).astype(np.int16)
    raster_f = raster_i.astype(np.float32) + np.random.default_rng(31).random(n, dtype=np.float32)
    print("raster %d x %d: values %d .. %d" % (rows, cols, raster_i.min(), raster_i.max()), file=sys.stderr, flush=True)
    blocks = {"int": (R.INT, raster_i), "short": (R.SHORT, raster_s), "float": (R.FLOAT, raster_f)}
    dev = {k: DeviceBuffer(ctx, v.nbytes + 16).upload(v) for k, (_, v) in blocks.items()}
    d_copy = DeviceBuffer(ctx, raster_i.nbytes + 16)
    results, agree = {}, {}

    # ---- the dense form
    n_bins = max(R.plan(*K.REF_RANGE)["n_bins"], R.plan(*GLOBAL_RANGE)["n_bins"])
    assert R.plan(*K.REF_RANGE)["n_bins"] <= K.LDS_MAX_BINS < R.plan(*GLOBAL_RANGE)["n_bins"]
    d_counter, d_summary = DeviceBuffer(ctx, n_bins * 4 + 16), DeviceBuffer(ctx, TAB_SUMMARY.itemsize)

    def dense(kind, window):
        ctx.tabulate_dense_dev(kind, dev[kind].ptr, n, *window, d_counter.ptr, d_summary.ptr)

    def copy_d2d(kind):
        assert hip.hipMemcpyAsync(d_copy.ptr, dev[kind].ptr, blocks[kind][1].nbytes, 3, stream) == 0      # hipMemcpyDeviceToDevice

    dense_cases = {"dense_short_ref": ("short", K.REF_RANGE), "dense_int_ref": ("int", K.REF_RANGE), "dense_int_global": ("int", GLOBAL_RANGE)}
    host_ms = {}
    for name, (kind, window) in dense_cases.items():
        elem_type, v = blocks[kind]
        wall = []
        for _ in range(HOST_REPS if name != "dense_int_global" else 1):
            t0 = time.perf_counter()
            want = K.harness_dense(th, v, elem_type, *window, threads=HOST_THREADS)
            wall.append((time.perf_counter() - t0) * 1e3)
        host_ms["host_" + name[6:]] = _stats(wall)
        check(L.gf_dev_memset(ctx.handle, d_counter.ptr, 0xA5, n_bins * 4), "gf_dev_memset")
        dense(kind, window)
        ctx.synchronize()
        got = d_counter.download(np.int32, want[0].size), K.summary_dict(d_summary.download(TAB_SUMMARY, 1))
        agree[name] = bool(np.array_equal(got[0], want[0]) and R.same_summary(got[1], want[1]))
        print("%s: equals the harness: %s; %d of %d cells counted, min %g at %d, max %g at %d" % (
            name, agree[name], got[1]["n_samples"], n, got[1]["min"], got[1]["min_at"], got[1]["max"], got[1]["max_at"]), file=sys.stderr, flush=True)
    cases = {name: (lambda kind=kind, window=window: dense(kind, window)) for name, (kind, window) in dense_cases.items()}
    cases["copy_d2d_short"], cases["copy_d2d_int"] = (lambda: copy_d2d("short")), (lambda: copy_d2d("int"))
    results.update(_timed(timer, cases, REPS))
    results.update(host_ms)
    for name, (kind, _) in dense_cases.items():
        results[name]["over_copy_d2d"] = round(results[name]["median_ms"] / results["copy_d2d_" + kind]["median_ms"], 3)

    # ---- the symbol form
    d_sym, d_cnt, d_ssum = DeviceBuffer(ctx, n * 4 + 16), DeviceBuffer(ctx, n * 4 + 16), DeviceBuffer(ctx, TAB_SYMBOLS.itemsize)
    temp_bytes = C.c_size_t()
    assert Y.tr_sort_temp_bytes(n, C.byref(temp_bytes)) == 0
    d_temp = DeviceBuffer(ctx, temp_bytes.value + 16)

    def symbols(kind, cells=n):
        ctx.tabulate_symbols_dev(kind, dev[kind].ptr, cells, d_sym.ptr, d_cnt.ptr, cells, d_ssum.ptr)

    def rocprim_sort(kind):
        assert Y.tr_sort(d_temp.ptr, temp_bytes.value, dev[kind].ptr, d_copy.ptr, n, stream) == 0

    def summary():
        s = d_ssum.download(TAB_SYMBOLS, 1)
        return {k: s[k][0].item() for k in TAB_SYMBOLS.names}

    part = min(n, 1 << 22)
    for kind in ("int", "float"):
        elem_type, v = blocks[kind]
        symbols(kind, part)
        ctx.synchronize()
        want = R.symbols(v[:part], elem_type)
        s = summary()
        k = want[2]["n_symbols"]
        agree["symbols_%s_first_%d_cells" % (kind, part)] = bool(s == want[2] and np.array_equal(d_sym.download(np.uint32, k), want[0]) and
                                                               np.array_equal(d_cnt.download(np.int32, k), want[1]))
        symbols(kind)
        ctx.synchronize()
        s = summary()
        ok = s["n_samples"] == n and s["n_unique"] + s["n_repeated"] == s["n_symbols"] == s["n_written"]
        if kind == "int":
            lo = int(raster_i.min())
            counts = np.bincount((raster_i.astype(np.int64) - lo).astype(np.int64))
            sym = (np.flatnonzero(counts) + lo).astype(np.int32).view(np.uint32)
            order = np.argsort(sym, kind="stable")
            k = s["n_symbols"]
            ok = ok and k == sym.size and np.array_equal(d_sym.download(np.uint32, k), sym[order]) and \
                np.array_equal(d_cnt.download(np.int32, k), counts[counts > 0][order].astype(np.int32)) and s["max_count"] == counts.max()
        agree["symbols_" + kind] = bool(ok)
        results["symbols_" + kind + "_summary"] = s
        print("symbols_%s: %s; %s" % (kind, {k: v for k, v in agree.items() if k.startswith("symbols_" + kind)}, s), file=sys.stderr, flush=True)
    cases = {"symbols_int": lambda: symbols("int"), "rocprim_sort_int": lambda: rocprim_sort("int"),
             "symbols_float": lambda: symbols("float"), "rocprim_sort_float": lambda: rocprim_sort("float")}
    results.update(_timed(timer, cases, SYM_REPS))
    for kind in ("int", "float"):
        results["symbols_" + kind]["over_rocprim_sort"] = round(results["symbols_" + kind]["median_ms"] / results["rocprim_sort_" + kind]["median_ms"], 2)
    for k, v in results.items():
        if "median_ms" in v and not k.startswith("host_"):
            kind = "short" if "short" in k else "float" if "float" in k else "int"
            v["source_GBps"] = round(blocks[kind][1].nbytes / 1e9 / (v["median_ms"] / 1e3), 1)             # bytes of the block per second
    out = {"workload": "etopo1 shape: a block of %d x %d cells from gf_synth_dem_dev as SHORT, INT and (with a fractional part) FLOAT" % (rows, cols),
           "method": "HIP events, warm-up, %d (dense, copies) / %d (symbols, rocprim) timings per case taken in turn in one process; host: wall "
                     "clock, %d timings, %d threads" % (REPS, SYM_REPS, HOST_REPS, HOST_THREADS),
           "csrc_digest": hipbuild.csrc_digest(), "cells": n, "thresholds": K.CONST,
           "results_equal_the_harness_or_the_model_bit_for_bit": agree, "cases": results}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
