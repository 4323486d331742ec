"""What accumulating the symbol table of a raster strip by strip costs: the ETOPO1-shaped block, 10,800 x 21,600 cells from
gf_synth_dem_dev (the method and the block of tools/tabulate_rate.py).
    python tools/tabulate_acc_rate.py [--out profiles/tabulate_acc_rate.json] [--shrink K]
HIP events on the context's stream, warm-up, then 7 timings per case taken in turn in one process; medians, min and max (the
spread).  Before the timings the table of the 8 strips is compared entry for entry with the table of the one call, the SHORT table
of the counters with the table of the sort.
  symbols_int / symbols_float      the yardstick: the unchanged gf_block_tabulate_symbols_dev over the whole raster in one call
  acc8_int / acc8_float            the raster in 8 strips through gf_block_tabulate_symbols_acc_dev, two tables taking turns
  copy_acc8_*                      device-to-device copies that move the bytes the eight merges read and write (a copy of x bytes
                                   reads x and writes x): the allowance over the yardstick, with the yardstick's own spread
  merge_float_halves               gf_tab_symbols_merge_dev of the tables of the FLOAT raster's two halves; copy_merge_float_halves:
                                   the copy that moves the same bytes
  short_counters                   gf_block_tabulate_symbols_acc_dev of the SHORT raster onto an empty table: k_tab_short_counts,
                                   k_tab_short_compact and the merge with nothing
  short_fixed_part                 the same call on one cell: the zeroing of the counters, the compaction and that merge
  dense_short_ref                  the yardstick: k_tabulate_dense on the same SHORT block with the reference's window
  symbols_short                    the one-call SHORT route, which widens and sorts in four passes
No threshold is enforced: the aims are written out with the numbers, and a miss reads ABOVE.  --shrink K divides both sides of the
block by K (a quick look)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gridfour_amd  # noqa: E402
from gridfour_amd import DeviceBuffer, DeviceTileBatch  # noqa: E402
from gridfour_amd import build as hipbuild  # noqa: E402
from gridfour_amd.codec import TAB_SUMMARY, TAB_SYMBOLS  # noqa: E402
import tabulate_acc_cases as KA  # noqa: E402
import tabulate_cases as K  # noqa: E402
from tabulate_rate import N_COLS, N_ROWS, TILE_ROWS, TILES_ACROSS, _hip, _stats, _timed  # noqa: E402

REPS, STRIPS = 7, 8


class Table:
    """a table in device memory with room for cap entries"""

    def __init__(self, ctx, cap):
        self.cap = cap
        self.sym, self.cnt, self.sum = DeviceBuffer(ctx, cap * 4 + 16), DeviceBuffer(ctx, cap * 4 + 16), DeviceBuffer(ctx, TAB_SYMBOLS.itemsize)

    def out(self):
        return self.sym.ptr, self.cnt.ptr, self.cap, self.sum.ptr

    def into(self):
        return self.sym.ptr, self.cnt.ptr, self.sum.ptr, self.cap

    def summary(self):
        s = self.sum.download(TAB_SYMBOLS, 1)
        return {k: s[k][0].item() for k in TAB_SYMBOLS.names}

    def entries(self):
        n = self.summary()["n_written"]
        return self.sym.download(np.uint32, n), self.cnt.download(np.int32, n)


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    shrink = int(argv[argv.index("--shrink") + 1]) if "--shrink" in argv else 1
    tile_rows, tiles_across = max(TILE_ROWS // shrink, 1), max(TILES_ACROSS // shrink, 1)
    nt = tile_rows * tiles_across
    hip = _hip()
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
    blocks = {"int": raster_i, "short": np.clip(raster_i, -32767, 32767).astype(np.int16),
              "float": raster_i.astype(np.float32) + np.random.default_rng(31).random(n, dtype=np.float32)}
    dev = {k: DeviceBuffer(ctx, v.nbytes + 16).upload(v) for k, v in blocks.items()}
    item = {k: v.itemsize for k, v in blocks.items()}
    one, ping, pong = Table(ctx, n), Table(ctx, n), Table(ctx, n)
    d_from, d_to = DeviceBuffer(ctx, 8 * n + 16), DeviceBuffer(ctx, 8 * n + 16)
    cuts = [n * k // STRIPS | 1 if 0 < k < STRIPS else n * k // STRIPS for k in range(STRIPS + 1)]      # odd cuts: SHORT strips at odd cells
    results, agree, moved = {}, {}, {}

    def one_call(kind):
        ctx.tabulate_symbols_dev(kind, dev[kind].ptr, n, *one.out())

    def strip_ptr(kind, a):
        return C.c_void_p(dev[kind].ptr.value + a * item[kind])

    def acc8(kind):
        into, tables = (None, None, None, 0), (ping, pong)
        for k in range(STRIPS):
            ctx.tabulate_symbols_acc_dev(kind, strip_ptr(kind, cuts[k]), cuts[k + 1] - cuts[k], *into, *tables[k & 1].out())
            into = tables[k & 1].into()
        return tables[(STRIPS - 1) & 1]

    def copies(sizes):
        for x in sizes:
            assert hip.hipMemcpyAsync(d_to.ptr, d_from.ptr, x, 3, stream) == 0                          # hipMemcpyDeviceToDevice

    # ---- INT and FLOAT: 8 strips against one call
    for kind in ("int", "float"):
        one_call(kind)
        last = acc8(kind)
        ctx.synchronize()
        s1, s8 = one.summary(), last.summary()
        (sym1, cnt1), (sym8, cnt8) = one.entries(), last.entries()
        agree["acc8_" + kind] = bool(s1 == s8 and np.array_equal(sym1, sym8) and np.array_equal(cnt1, cnt8))
        results["symbols_%s_summary" % kind] = s1
        # the entries each merge reads (the in-table, the strip's table) and writes: a strip's own table by the one-call form
        sizes, n_in = [], 0
        for k in range(STRIPS):
            ctx.tabulate_symbols_dev(kind, strip_ptr(kind, cuts[k]), cuts[k + 1] - cuts[k], None, None, 0, one.sum.ptr)
            ctx.synchronize()
            n_strip = one.summary()["n_symbols"]
            ctx.tabulate_symbols_acc_dev(kind, strip_ptr(kind, cuts[k]), cuts[k + 1] - cuts[k],
                                         *((None, None, None, 0) if k == 0 else (ping, pong)[(k - 1) & 1].into()), *(ping, pong)[k & 1].out())
            ctx.synchronize()
            n_out = (ping, pong)[k & 1].summary()["n_symbols"]
            sizes.append((n_in + n_strip + n_out) * 8 // 2 // 16 * 16)
            n_in = n_out
        moved[kind] = sizes
        print("%s: 8 strips equal one call: %s; %s; merges move %s bytes" % (kind, agree["acc8_" + kind], s1, [2 * x for x in sizes]),
              file=sys.stderr, flush=True)
    cases = {}
    for kind in ("int", "float"):
        cases["symbols_" + kind] = lambda kind=kind: one_call(kind)
        cases["acc8_" + kind] = lambda kind=kind: acc8(kind)
        cases["copy_acc8_" + kind] = lambda kind=kind: copies(moved[kind])
    results.update(_timed(timer, cases, REPS))

    # ---- the merge alone: the tables of the FLOAT raster's two halves
    half = n // 2
    ctx.tabulate_symbols_dev("float", dev["float"].ptr, half, *ping.out())
    ctx.tabulate_symbols_dev("float", strip_ptr("float", half), n - half, *pong.out())
    ctx.tabulate_symbols_dev("float", dev["float"].ptr, n, None, None, 0, d_to.ptr)                      # (the whole raster's scalars)
    ctx.tab_symbols_merge_dev(*ping.into(), *pong.into(), *one.out())
    ctx.synchronize()
    whole, merged = d_to.download(TAB_SYMBOLS, 1), one.summary()
    agree["merge_float_halves"] = bool(all(merged[k] == whole[k][0].item() for k in TAB_SYMBOLS.names if k != "n_written"))
    merge_bytes = (ping.summary()["n_written"] + pong.summary()["n_written"] + merged["n_written"]) * 8
    cases = {"merge_float_halves": lambda: ctx.tab_symbols_merge_dev(*ping.into(), *pong.into(), *one.out()),
             "copy_merge_float_halves": lambda: copies([merge_bytes // 2 // 16 * 16])}
    results.update(_timed(timer, cases, REPS))
    results["merge_float_halves"]["bytes_moved"] = merge_bytes

    # ---- SHORT: counters and compaction against the dense form's kernel and the four-pass route
    d_counter, d_summary = DeviceBuffer(ctx, 19652 * 4 + 16), DeviceBuffer(ctx, TAB_SUMMARY.itemsize)
    one_call("short")
    ctx.tabulate_symbols_acc_dev("short", dev["short"].ptr, n, None, None, None, 0, *ping.out())
    ctx.synchronize()
    (sym1, cnt1), (symc, cntc) = one.entries(), ping.entries()
    agree["short_counters"] = bool(one.summary() == ping.summary() and np.array_equal(sym1, symc) and np.array_equal(cnt1, cntc))
    cases = {"short_counters": lambda: ctx.tabulate_symbols_acc_dev("short", dev["short"].ptr, n, None, None, None, 0, *ping.out()),
             "short_fixed_part": lambda: ctx.tabulate_symbols_acc_dev("short", dev["short"].ptr, 1, None, None, None, 0, *pong.out()),
             "dense_short_ref": lambda: ctx.tabulate_dense_dev("short", dev["short"].ptr, n, *K.REF_RANGE, d_counter.ptr, d_summary.ptr),
             "symbols_short": lambda: one_call("short")}
    results.update(_timed(timer, cases, REPS))

    # ---- the aims
    spread = lambda k: results[k]["max_ms"] - results[k]["min_ms"]
    aims = {}
    for kind in ("int", "float"):
        bound = results["symbols_" + kind]["median_ms"] + results["copy_acc8_" + kind]["median_ms"] + spread("symbols_" + kind)
        got = results["acc8_" + kind]["median_ms"]
        aims["acc8_" + kind] = {"median_ms": got, "allowed_ms": round(bound, 4), "over_one_call": round(got / results["symbols_" + kind]["median_ms"], 3),
                                "verdict": "within" if got <= bound else "ABOVE"}
    got, copy = results["merge_float_halves"]["median_ms"], results["copy_merge_float_halves"]["median_ms"]
    aims["merge_float_halves"] = {"median_ms": got, "copy_ms": copy, "over_copy": round(got / copy, 2)}
    bound = results["dense_short_ref"]["median_ms"] + spread("dense_short_ref") + results["short_fixed_part"]["median_ms"]
    got = results["short_counters"]["median_ms"]
    aims["short_counters"] = {"median_ms": got, "allowed_ms": round(bound, 4), "over_dense": round(got / results["dense_short_ref"]["median_ms"], 3),
                              "four_pass_route_ms": results["symbols_short"]["median_ms"],
                              "four_pass_over_counters": round(results["symbols_short"]["median_ms"] / got, 1),
                              "verdict": "within" if got <= bound else "ABOVE"}
    out = {"workload": "etopo1 shape: a block of %d x %d cells from gf_synth_dem_dev as INT, SHORT and (with a fractional part) FLOAT; "
                       "%d strips cut at odd cells" % (rows, cols, STRIPS),
           "method": "HIP events, warm-up, %d timings per case taken in turn in one process; spread = max - min" % REPS,
           "csrc_digest": hipbuild.csrc_digest(), "cells": n, "constants": KA.CONST, "results_equal": agree, "aims": aims, "cases": results}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
