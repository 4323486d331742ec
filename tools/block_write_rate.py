"""What a block write costs beside the two calls it composes and beside a plain copy of the raster's bytes: the ETOPO1 shape, a
10,800 x 21,600 grid under tiles of 120 x 150 cells (12,960 tiles), the whole grid as one rectangle.
    python tools/block_write_rate.py [--out profiles/block_write_rate.json] [--tile-rows 90]
HIP events on the context's stream, list (CodecCanonHuffman,), checksums on, 20 timings per case taken in turn in one process;
medians, min and max.  Before the timings the outputs of the cases that must agree are compared byte for byte.
  (a) what a caller could do before: gf_tiles_from_block_dev followed by gf_tile_record_encode_batch_elems_dev, one INT element
  (b) gf_block_write_elems_dev on the same raster
  (c) the same for a SHORT and an int-coded-float element: (c1) gf_block_write_elems_dev on int16 cells and float VALUES; (c0) by
      hand, two cuts and the record write, with the ICF codes prepared on the host OUTSIDE the timed region -- the wall time of that
      host conversion (numpy, range checks included) is reported beside it
  (d) the cut stage alone (the flags' memset, k_block_cut_elems, k_block_write_verdict) for the INT raster, through a hook that only
      the diagnostic flavour of the library has (libgvrs_hip_diag.so, loaded beside the shipping library for this case alone, with a
      context of its own, on the timed stream), against (e) a device-to-device hipMemcpyAsync of the raster's bytes and (f)
      gf_tiles_from_block_dev, the plain cut of the same raster, in the same run
Condition:  median(b) <= median(a) + spread(a)  (spread = max - min of (a) in this run).  The values and the verdict are written
as they come out; nothing here asserts them."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gridfour_amd  # noqa: E402
from gridfour_amd import DeviceBuffer, DeviceTileBatch, lib  # noqa: E402
from gridfour_amd._lib import check  # noqa: E402
from gridfour_amd.codec import _ELEM_SPEC  # noqa: E402

REPS = 20
CODECS = [3]
N_ROWS, N_COLS, TILES_ACROSS = 120, 150, 144
INT, SHORT, ICF = 0, 1, 3
ICF_SCALE, ICF_OFFSET = 10.0, -100.0


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


class Out:
    """the output arrays of one record write in device memory"""

    def __init__(self, ctx, nt, ne, cap):
        self.nt, self.ne, self.cap = nt, ne, cap
        self.blob = DeviceBuffer(ctx, cap + 64)
        self.off = DeviceBuffer(ctx, (nt + 1) * 8 + 16)
        self.idx = DeviceBuffer(ctx, nt * 4 + 16)
        self.used = DeviceBuffer(ctx, ne * nt + 16)
        self.st = DeviceBuffer(ctx, nt * 4 + 16)

    def get(self):
        off = self.off.download(np.uint64, self.nt + 1)
        return (self.blob.download(np.uint8, int(off[-1])), off, self.idx.download(np.int32, self.nt), self.used.download(np.uint8, self.ne * self.nt),
                self.st.download(np.int32, self.nt))

    def free(self):
        for b in (self.blob, self.off, self.idx, self.used, self.st):
            b.free()


def _same(a, b, what):
    for x, y, name in zip(a, b, ("blob", "offsets", "indices", "codec_used", "status")):
        assert np.array_equal(x, y), (what, name)


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    tile_rows = int(argv[argv.index("--tile-rows") + 1]) if "--tile-rows" in argv else 90
    nt, cells = tile_rows * TILES_ACROSS, N_ROWS * N_COLS
    L, hip = lib(), _hip()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    ctx = gridfour_amd.GvrsHipContext(0)
    b = DeviceTileBatch(ctx, N_ROWS, N_COLS, nt, slot_stride=16)
    b.synth_dem(0x9E3779B97F4A7C15 + 2, TILES_ACROSS)
    ctx.synchronize()
    vals = b.get_values().reshape(nt, cells)
    b.free()
    rows, cols = tile_rows * N_ROWS, TILES_ACROSS * N_COLS
    raster_i = np.ascontiguousarray(vals.reshape(tile_rows, TILES_ACROSS, N_ROWS, N_COLS).transpose(0, 2, 1, 3).reshape(rows, cols))
    raster_s = np.clip(raster_i, -32767, 32767).astype(np.int16)
    raster_f = (raster_s.astype(np.float32) / np.float32(ICF_SCALE) + np.float32(ICF_OFFSET)).astype(np.float32)
    # the host's share of the by-hand path: TileElementIntCodedFloat.setValue over the raster, in numpy
    t0 = time.perf_counter()
    lo = np.float32(-2 ** 31 + 1) / np.float32(ICF_SCALE) + np.float32(ICF_OFFSET)
    hi = np.float32(2 ** 31 - 2) / np.float32(ICF_SCALE) + np.float32(ICF_OFFSET)
    is_fill = np.isnan(raster_f)
    assert bool(((raster_f >= lo) & (raster_f <= hi) | is_fill).all())
    d = (raster_f - np.float32(ICF_OFFSET)) * np.float32(ICF_SCALE)
    codes = np.where(is_fill, -2 ** 31, np.clip(np.floor(d.astype(np.float64) + 0.5), -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int32)
    host_ms = (time.perf_counter() - t0) * 1e3
    grid = np.array([rows, cols, N_ROWS, N_COLS], np.int32)
    rect = np.array([0, 0, rows, cols], np.int32)
    cd = (C.c_int * len(CODECS))(*CODECS)
    idx = np.arange(nt, dtype=np.int32)
    timer = gridfour_amd.GpuTimer(ctx)
    stream = C.c_void_p(ctx.stream)

    spec1 = np.zeros(1, _ELEM_SPEC)
    spec1["type"], spec1["scale"], spec1["fill_i"] = INT, 1.0, -2 ** 31
    spec2 = np.zeros(2, _ELEM_SPEC)
    spec2["type"] = [SHORT, ICF]
    spec2["scale"], spec2["offset"] = [1.0, ICF_SCALE], [0.0, ICF_OFFSET]
    spec2["fill_i"], spec2["fill_f"] = [-32768, -2 ** 31], [0.0, np.nan]
    cap1 = nt * int(L.gf_tile_record_max_bytes_elems(_p(spec1), 1, N_ROWS, N_COLS))
    cap2 = nt * int(L.gf_tile_record_max_bytes_elems(_p(spec2), 2, N_ROWS, N_COLS))

    d_ri = DeviceBuffer(ctx, raster_i.nbytes + 16).upload(raster_i)
    d_rs = DeviceBuffer(ctx, raster_s.nbytes + 16).upload(raster_s)
    d_rf = DeviceBuffer(ctx, raster_f.nbytes + 16).upload(raster_f)
    d_rc = DeviceBuffer(ctx, codes.nbytes + 16).upload(codes)
    d_copy = DeviceBuffer(ctx, raster_i.nbytes + 16)
    d_t0 = DeviceBuffer(ctx, nt * cells * 4 + 16)
    d_t1 = DeviceBuffer(ctx, nt * cells * 4 + 16)
    d_idx = DeviceBuffer(ctx, nt * 4 + 16).upload(idx)
    oa, ob, oc0, oc1 = Out(ctx, nt, 1, cap1), Out(ctx, nt, 1, cap1), Out(ctx, nt, 2, cap2), Out(ctx, nt, 2, cap2)
    p_t1 = (C.c_void_p * 1)(d_t0.ptr.value)
    p_t2 = (C.c_void_p * 2)(d_t0.ptr.value, d_t1.ptr.value)
    p_b1 = (C.c_void_p * 1)(d_ri.ptr.value)
    p_b2 = (C.c_void_p * 2)(d_rs.ptr.value, d_rf.ptr.value)
    from gridfour_amd import build as hipbuild
    diag = C.CDLL(hipbuild.LIB_DIAG)                                    # (built beside the shipping library; only its cut hook is used)
    diag.gf_context_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    diag_ctx = C.c_void_p()
    check(diag.gf_context_create(0, C.byref(diag_ctx)), "gf_context_create (diagnostic library)")
    cut_hook = diag.gf_internal_block_cut_elems_dev
    cut_hook.restype = C.c_int
    cut_hook.argtypes = [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4

    def a_by_hand():
        check(L.gf_tiles_from_block_dev(ctx.handle, None, _p(grid), _p(rect), INT, 0x80000000, 0, d_ri.ptr, nt, d_idx.ptr, d_t0.ptr, None),
              "gf_tiles_from_block_dev")
        check(L.gf_tile_record_encode_batch_elems_dev(ctx.handle, None, cd, len(CODECS), _p(spec1), 1, N_ROWS, N_COLS, nt, d_idx.ptr, p_t1, 1,
                                                      oa.blob.ptr, cap1, oa.off.ptr, oa.used.ptr, oa.st.ptr), "gf_tile_record_encode_batch_elems_dev")

    def b_block_write():
        check(L.gf_block_write_elems_dev(ctx.handle, None, cd, len(CODECS), _p(spec1), None, 1, _p(grid), _p(rect), p_b1, 0, None, 0, None, 0, 1,
                                         ob.blob.ptr, cap1, ob.off.ptr, ob.idx.ptr, ob.used.ptr, ob.st.ptr), "gf_block_write_elems_dev")

    def c0_by_hand():
        check(L.gf_tiles_from_block_dev(ctx.handle, None, _p(grid), _p(rect), SHORT, 0x8000, 0, d_rs.ptr, nt, d_idx.ptr, d_t0.ptr, None),
              "gf_tiles_from_block_dev")
        check(L.gf_tiles_from_block_dev(ctx.handle, None, _p(grid), _p(rect), INT, 0x80000000, 0, d_rc.ptr, nt, d_idx.ptr, d_t1.ptr, None),
              "gf_tiles_from_block_dev")
        check(L.gf_tile_record_encode_batch_elems_dev(ctx.handle, None, cd, len(CODECS), _p(spec2), 2, N_ROWS, N_COLS, nt, d_idx.ptr, p_t2, 1,
                                                      oc0.blob.ptr, cap2, oc0.off.ptr, oc0.used.ptr, oc0.st.ptr), "gf_tile_record_encode_batch_elems_dev")

    def c1_block_write():
        check(L.gf_block_write_elems_dev(ctx.handle, None, cd, len(CODECS), _p(spec2), None, 2, _p(grid), _p(rect), p_b2, 0, None, 0, None, 0, 1,
                                         oc1.blob.ptr, cap2, oc1.off.ptr, oc1.idx.ptr, oc1.used.ptr, oc1.st.ptr), "gf_block_write_elems_dev")

    def d_cut_alone():
        check(cut_hook(diag_ctx, stream, _p(spec1), None, 1, _p(grid), _p(rect), p_b1, ob.idx.ptr), "gf_internal_block_cut_elems_dev")

    def f_plain_cut():
        check(L.gf_tiles_from_block_dev(ctx.handle, None, _p(grid), _p(rect), INT, 0x80000000, 0, d_ri.ptr, nt, d_idx.ptr, d_t0.ptr, None),
              "gf_tiles_from_block_dev")

    def e_copy():
        assert hip.hipMemcpyAsync(d_copy.ptr, d_ri.ptr, raster_i.nbytes, 3, stream) == 0          # hipMemcpyDeviceToDevice

    # every case once outside the timings (the context's buffers grow, code objects load); outputs that must agree are compared
    for fn in (a_by_hand, b_block_write, c0_by_hand, c1_block_write, d_cut_alone, e_copy, f_plain_cut):
        fn()
    ctx.synchronize()
    oa.idx.upload(idx)
    oc0.idx.upload(idx)
    ga, gb, gc0, gc1 = oa.get(), ob.get(), oc0.get(), oc1.get()
    assert (gb[4] == 0).all() and (gc1[4] == 0).all()
    _same(ga, gb, "one INT element")
    _same(gc0, gc1, "SHORT + ICF")
    r = _series(timer, {"a_cut_then_record_write": a_by_hand, "b_block_write_elems_dev": b_block_write, "c0_short_icf_by_hand": c0_by_hand,
                        "c1_short_icf_block_write": c1_block_write, "d_cut_stage_alone": d_cut_alone, "e_copy_d2d": e_copy, "f_tiles_from_block_dev": f_plain_cut})
    ctx.synchronize()
    _same(oa.get(), ob.get(), "one INT element, after the timings")
    a, bb = r["a_cut_then_record_write"], r["b_block_write_elems_dev"]
    limit = a["median_ms"] + a["spread_ms"]
    for k in ("d_cut_stage_alone", "e_copy_d2d", "f_tiles_from_block_dev"):
        r[k]["GBps_of_raster"] = round(raster_i.nbytes / 1e9 / (r[k]["median_ms"] / 1e3), 1)
    out = {"workload": "etopo1 shape: a raster of %d x %d cells written as one block under tiles of %dx%d cells (%d tiles)" % (rows, cols, N_ROWS,
                                                                                                                         N_COLS, nt),
           "codec_list": CODECS, "method": "HIP events, %d timings per case taken in turn in one process, checksums on" % REPS,
           "csrc_digest": gridfour_amd.build.csrc_digest() if hasattr(gridfour_amd, "build") else None,
           "raster_bytes_int": int(raster_i.nbytes), "record_bytes_int": int(ga[1][-1]), "record_bytes_short_icf": int(gc0[1][-1]),
           "host_icf_conversion_wall_ms": round(host_ms, 1), "cases": r,
           "conditions": {"b_le_a_plus_spread_a": {"value_ms": bb["median_ms"], "limit_ms": round(limit, 4), "holds": bool(bb["median_ms"] <= limit)}}}
    diag.gf_context_destroy.argtypes = [C.c_void_p]
    diag.gf_context_destroy(diag_ctx)
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
