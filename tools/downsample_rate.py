"""What downsampling a device-resident block costs: the ETOPO1-shaped block, 10,800 x 21,600 cells, as FLOAT, INT and SHORT, averaged
down by the factors 2, 3, 4, 8 and 60.
    python tools/downsample_rate.py [--out profiles/downsample_rate.json] [--shrink K]
HIP events on the context's stream, 20 timings per case taken in turn in one process; medians, min and max.  Before the timings the
output of each kernel path is compared bit for bit with the CPU harness (tests/csrc/downsample_harness.cpp).
  direct / staged    gf_block_downsample_elems_dev with k_downsample_direct / k_downsample_staged forced (the diagnostic flavour of
                     the library, gf_internal_downsample_path); "auto" names the path the shipping library takes
  copy_d2d           a device-to-device copy of the input block's bytes: the memory yardstick (it reads AND writes them)
  host               what a caller had before: the block copied to the host, the stand-alone C++ harness (g++ -O2
                     -ffp-contract=off) on 16 threads, the result copied back; wall clock, 3 timings
No threshold is set: the numbers are written as they come out.  --shrink K divides both sides of the block by K (a quick look)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

os.environ["GVRS_HIP_DIAG"] = "1"          # the diagnostic flavour: the same kernels, and the hook that forces a path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gridfour_amd  # noqa: E402
from gridfour_amd import DeviceBuffer, lib  # noqa: E402
from gridfour_amd import build as hipbuild  # noqa: E402
from gridfour_amd._lib import check  # noqa: E402
from gridfour_amd.codec import _ELEM_SPEC  # noqa: E402
import downsample_cases as K  # noqa: E402
import downsample_ref as R  # noqa: E402

REPS, HOST_REPS, HOST_THREADS = 20, 3, 16
FACTORS = (2, 3, 4, 8, 60)
AUTO, DIRECT, STAGED = 0, 1, 2
FILL = {R.FLOAT: 0, R.INT: -2 ** 31, R.SHORT: -32768}


def _hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("libamdhip64 not loadable")


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _stats(v, reps):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": reps}


def _block(rng, elem_type, shape):
    """terrain-like magnitudes; no fill cells (a fill would only shorten the work: the loads are the same)"""
    v = rng.standard_normal(shape, dtype=np.float32) * np.float32(1000.0)
    return v if elem_type == R.FLOAT else v.astype(R.DTYPES[elem_type])


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    shrink = int(argv[argv.index("--shrink") + 1]) if "--shrink" in argv else 1
    n_rows, n_cols = 10800 // shrink, 21600 // shrink
    rect = (0, 0, n_rows, n_cols)
    L, hip = lib(), _hip()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    force = L.gf_internal_downsample_path
    force.argtypes, force.restype = [C.c_int], None
    dh = K.build_harness()
    ctx = gridfour_amd.GvrsHipContext(0)
    timer = gridfour_amd.GpuTimer(ctx)
    stream = C.c_void_p(ctx.stream)
    rng = np.random.default_rng(30)
    results, agree = {}, {}
    for elem_type in (R.FLOAT, R.INT, R.SHORT):
        name = K.KINDS[elem_type]
        block = _block(rng, elem_type, (n_rows, n_cols))
        spec = np.zeros(1, _ELEM_SPEC)
        spec["type"], spec["fill_i"] = elem_type, FILL[elem_type]
        d_block = DeviceBuffer(ctx, block.nbytes + 16).upload(block)
        d_copy = DeviceBuffer(ctx, block.nbytes + 16)
        d_out = DeviceBuffer(ctx, block.nbytes // 4 + 16)
        h_block = np.empty_like(block)
        print("%s block uploaded" % name, file=sys.stderr, flush=True)

        def copy_d2d():
            assert hip.hipMemcpyAsync(d_copy.ptr, d_block.ptr, block.nbytes, 3, stream) == 0      # hipMemcpyDeviceToDevice

        for f in FACTORS:
            out_shape = R.out_rect(rect, f)[2:]
            n_out = out_shape[0] * out_shape[1]
            g = K.geom_of(rect, f, elem_type, FILL[elem_type])
            h_out = np.empty(out_shape, block.dtype)

            def device(path):
                force(path)
                ctx.downsample_dev(spec, rect, f, [d_block.ptr], [d_out.ptr])
                force(AUTO)

            def host_route():
                check(L.gf_dev_download(ctx.handle, _p(h_block), d_block.ptr, block.nbytes), "gf_dev_download")
                dh.dh_downsample(_p(g), _p(h_block), _p(h_out), HOST_THREADS)
                check(L.gf_dev_upload(ctx.handle, d_out.ptr, _p(h_out), h_out.nbytes), "gf_dev_upload")

            # every path once outside the timings: each must equal the harness in every bit
            host_route()
            want = h_out.copy()
            same = {}
            for key, path in (("direct", DIRECT), ("staged", STAGED), ("auto", AUTO)):
                check(L.gf_dev_memset(ctx.handle, d_out.ptr, 0xA5, n_out * block.itemsize), "gf_dev_memset")
                device(path)
                ctx.synchronize()
                same[key] = R.same_bits(d_out.download(block.dtype, n_out).reshape(out_shape), want)
            agree["%s_f%d" % (name, f)] = same
            copy_d2d()
            ctx.synchronize()
            cases = {"direct": lambda: device(DIRECT), "staged": lambda: device(STAGED), "copy_d2d": copy_d2d}
            ms = {k: [] for k in cases}
            for _ in range(REPS):
                for k, fn in cases.items():
                    timer.start()
                    fn()
                    timer.stop()
                    ms[k].append(timer.elapsed_ms())
            r = {k: _stats(v, REPS) for k, v in ms.items()}
            wall = []
            for _ in range(HOST_REPS):
                t0 = time.perf_counter()
                host_route()
                wall.append((time.perf_counter() - t0) * 1e3)
            r["host"] = _stats(wall, HOST_REPS)
            for k, v in r.items():
                v["source_GBps"] = round(block.nbytes / 1e9 / (v["median_ms"] / 1e3), 1)      # bytes of the block read per second
            results["%s_f%d" % (name, f)] = r
            print("%s f = %d: %s; direct %.3f ms, staged %.3f ms, copy %.3f ms, host %.0f ms" % (
                name, f, same, r["direct"]["median_ms"], r["staged"]["median_ms"], r["copy_d2d"]["median_ms"], r["host"]["median_ms"]),
                file=sys.stderr, flush=True)
        for b in (d_block, d_copy, d_out):
            b.free()
    out = {"workload": "etopo1 shape: a block of %d x %d cells as FLOAT, INT and SHORT, box-averaged by %s" % (n_rows, n_cols, list(FACTORS)),
           "method": "HIP events, %d timings per case taken in turn in one process; host: wall clock, %d timings, %d threads" %
                     (REPS, HOST_REPS, HOST_THREADS),
           "csrc_digest": hipbuild.csrc_digest(), "cells": n_rows * n_cols,
           "outputs_equal_the_harness_bit_for_bit": agree, "cases": results}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
