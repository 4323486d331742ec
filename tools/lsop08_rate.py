"""What the LSOP08 stages cost beside their LSOP12 counterparts, on device-resident batches.
    python tools/lsop08_rate.py [--out profiles/lsop08_rate.json] [--shrink K]
Two batches: the ETOPO1-shaped one (12,960 tiles of 120 x 150 from gf_synth_dem_dev, as bench.py makes it) and the float256_lsop shape
(4,096 tiles of 256 x 256, the same surface as int-coded floats).  HIP events on the context's stream, REPS timings per case taken in
turn in one process after a warm-up call of each; medians, min and max.  Per batch and per stage -- predict, reconstruct, encode
(device form), decode (device form) -- the gf_lsop08_* call is timed beside the gf_lsop12_* call on the same tiles, and beside a
device-to-device copy of the tiles' bytes.  Compressed bytes per cell are reported for both codecs.
Before the timings every tile of both codecs is decoded and compared with its input, and eight tiles' LSOP08 packings are compared
with the Python restatement (tests/lsop08_ref.py).
aim: an LSOP08 stage takes no longer than the LSOP12 stage beside it -- its median within the LSOP12 median plus the spread
(max - min) of that stage's own timings.  No threshold is enforced: the numbers are written as they come out, with the verdict beside
them.  --shrink K divides the tile counts by K."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gridfour_amd  # noqa: E402
from gridfour_amd import DeviceBuffer, lib  # noqa: E402
from gridfour_amd import build as hipbuild  # noqa: E402
from gridfour_amd._lib import check  # noqa: E402
import lsop08_ref as R  # noqa: E402

REPS = 20
SEED = 0x9E3779B97F4A7C15
WORKLOADS = {          # rows, cols, tiles, tiles per row, seed offset (bench.py's)
    "etopo1": (120, 150, 12960, 144, 2),
    "float256_lsop": (256, 256, 4096, 64, 5),
}


def _hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("libamdhip64 not loadable")


def _stats(v):
    med = float(np.median(v))
    return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v)}


def _verdict(case, yard):
    """the aim: no longer than the LSOP12 stage, within that stage's own spread"""
    spread = yard["max_ms"] - yard["min_ms"]
    limit = yard["median_ms"] + spread
    return {"ratio_to_lsop12": round(case["median_ms"] / yard["median_ms"], 3), "lsop12_spread_ms": round(spread, 4),
            "limit_ms": round(limit, 4), "within_aim": bool(case["median_ms"] <= limit)}


class Side:
    """the work buffers of one codec on a batch"""

    def __init__(self, ctx, family, nr, nc, nt, stride):
        L = lib()
        self.family = family
        n = int(getattr(L, "gf_%s_residual_count" % family)(nr, nc))
        self.res_stride = (n + 3) // 4 * 4
        self.slots = DeviceBuffer(ctx, nt * stride + 16)
        self.lengths, self.enc_status, self.dec_status = DeviceBuffer(ctx, nt * 4), DeviceBuffer(ctx, nt * 4), DeviceBuffer(ctx, nt * 4)
        self.decoded = DeviceBuffer(ctx, nt * nr * nc * 4)
        self.residuals, self.coefs, self.scratch = DeviceBuffer(ctx, nt * self.res_stride * 4 + 16), DeviceBuffer(ctx, nt * 64), DeviceBuffer(ctx, nt * 4)
        self.pred_status = DeviceBuffer(ctx, nt * 4)

    def buffers(self):
        return [self.slots, self.lengths, self.enc_status, self.dec_status, self.decoded, self.residuals, self.coefs, self.scratch, self.pred_status]


def run_workload(name, shrink, ctx, timer, hip):
    nr, nc, nt, per_row, seed_off = WORKLOADS[name]
    nt = max(8, nt // shrink)
    cells = nr * nc
    L = lib()
    stride = ((2 * cells + 1024) + 15) // 16 * 16
    values = DeviceBuffer(ctx, nt * cells * 4)
    copy_dst = DeviceBuffer(ctx, nt * cells * 4)
    check(L.gf_synth_dem_dev(ctx.handle, None, (SEED + seed_off) & (2 ** 64 - 1), nr, nc, per_row, 0, nt, values.ptr), "gf_synth_dem_dev")
    ctx.synchronize()
    tiles = values.download(np.int32, nt * cells).reshape(nt, cells)
    if name == "float256_lsop":
        f = tiles.astype(np.float32) * np.float32(0.1)
        tiles = np.floor((f * np.float32(10.0)).astype(np.float64) + 0.5).astype(np.int32)
        values.upload(tiles)
    h = ctx.handle
    s8, s12 = Side(ctx, "lsop08", nr, nc, nt, stride), Side(ctx, "lsop12", nr, nc, nt, stride)

    def predict08():
        check(L.gf_lsop08_predict_dev(h, nr, nc, nt, values.ptr, s8.residuals.ptr, s8.res_stride, s8.coefs.ptr, s8.pred_status.ptr), "predict08")

    def predict12():
        check(L.gf_lsop12_predict_dev(h, None, nr, nc, nt, values.ptr, s12.residuals.ptr, s12.res_stride, s12.coefs.ptr, s12.pred_status.ptr), "predict12")

    def reconstruct08():
        check(L.gf_lsop08_reconstruct_dev(h, nr, nc, nt, s8.residuals.ptr, s8.res_stride, s8.coefs.ptr, s8.pred_status.ptr, s8.decoded.ptr,
                                          s8.dec_status.ptr), "reconstruct08")

    def reconstruct12():
        check(L.gf_lsop12_reconstruct_dev(h, None, nr, nc, nt, s12.residuals.ptr, s12.res_stride, s12.coefs.ptr, s12.pred_status.ptr, s12.decoded.ptr,
                                          s12.dec_status.ptr), "reconstruct12")

    def encode08():
        check(L.gf_lsop08_encode_batch_i32_dev(h, 0, nr, nc, nt, values.ptr, s8.slots.ptr, stride, s8.lengths.ptr, s8.enc_status.ptr, s8.residuals.ptr,
                                               s8.res_stride, s8.coefs.ptr, s8.scratch.ptr), "encode08")

    def encode12():
        check(L.gf_lsop12_encode_batch_i32_dev(h, None, 0, nr, nc, nt, values.ptr, s12.slots.ptr, stride, s12.lengths.ptr, s12.enc_status.ptr,
                                               s12.residuals.ptr, s12.res_stride, s12.coefs.ptr, s12.scratch.ptr), "encode12")

    def decode08():
        check(L.gf_lsop08_decode_batch_i32_dev(h, nr, nc, nt, s8.slots.ptr, nt * stride, None, stride, s8.lengths.ptr, s8.decoded.ptr, s8.dec_status.ptr,
                                               s8.residuals.ptr, s8.res_stride, s8.coefs.ptr, s8.scratch.ptr), "decode08")

    def decode12():
        check(L.gf_lsop12_decode_batch_i32_dev(h, None, nr, nc, nt, s12.slots.ptr, nt * stride, None, stride, s12.lengths.ptr, s12.decoded.ptr,
                                               s12.dec_status.ptr, s12.residuals.ptr, s12.res_stride, s12.coefs.ptr, s12.scratch.ptr), "decode12")

    def copy():
        assert hip.hipMemcpyAsync(copy_dst.ptr, values.ptr, nt * cells * 4, 3, C.c_void_p(ctx.stream)) == 0      # hipMemcpyDeviceToDevice

    # ---- every tile round-trips, through the stages and through the containers; eight packings against the restatement ----
    agree = {}
    for tag, side, fns in (("lsop08", s8, (predict08, reconstruct08, encode08, decode08)), ("lsop12", s12, (predict12, reconstruct12, encode12, decode12))):
        fns[0]()
        fns[1]()
        ctx.synchronize()
        ok = side.pred_status.download(np.int32, nt) == 0
        agree[tag + "_tiles_predicted"] = int(ok.sum())
        agree[tag + "_reconstruct_gives_the_tiles"] = bool(np.array_equal(side.decoded.download(np.int32, nt * cells).reshape(nt, cells)[ok], tiles[ok]))
        side.decoded.fill(0xA5)
        fns[2]()
        fns[3]()
        ctx.synchronize()
        enc_ok = side.enc_status.download(np.int32, nt) == 0
        dec = side.dec_status.download(np.int32, nt)
        agree[tag + "_tiles_encoded"] = int(enc_ok.sum())
        agree[tag + "_decode_gives_the_tiles"] = bool((dec[enc_ok] == 0).all() and
                                                      np.array_equal(side.decoded.download(np.int32, nt * cells).reshape(nt, cells)[enc_ok], tiles[enc_ok]))
        side.bytes_per_cell = float(side.lengths.download(np.uint32, nt)[enc_ok].sum()) / (max(1, int(enc_ok.sum())) * cells)
    lengths = s8.lengths.download(np.uint32, nt)
    same = 0
    sample = [int(t) for t in np.linspace(0, nt - 1, 8)]
    for t in sample:
        got = bytes(s8.slots.download(np.uint8, int(lengths[t]), t * stride))
        same += int(got == R.encode(0, nr, nc, tiles[t], force_type=0)[0])
    agree["lsop08_packings_equal_the_restatement"] = "%d of %d" % (same, len(sample))
    print("%s: checked %s" % (name, agree), file=sys.stderr, flush=True)

    # ---- the timings, in turn ----
    cases = {"predict08": predict08, "predict12": predict12, "reconstruct08": reconstruct08, "reconstruct12": reconstruct12, "encode08": encode08,
             "encode12": encode12, "decode08": decode08, "decode12": decode12, "copy": copy}
    for fn in cases.values():
        fn()
    ms = {k: [] for k in cases}
    for _ in range(REPS):
        for k, fn in cases.items():
            timer.start()
            fn()
            timer.stop()
            ctx.synchronize()
            ms[k].append(timer.elapsed_ms())
    st = {k: _stats(v) for k, v in ms.items()}
    raw = nt * cells * 4
    stages = {}
    for stage in ("predict", "reconstruct", "encode", "decode"):
        a, b = st[stage + "08"], st[stage + "12"]
        for x in (a, b):
            x["tile_GBps"] = round(raw / 1e9 / (x["median_ms"] / 1e3), 1)
        a.update(_verdict(a, b))
        stages[stage] = {"lsop08": a, "lsop12": b}
        print("%s %s: LSOP08 %.3f ms, LSOP12 %.3f ms (%.3f .. %.3f)" % (name, stage, a["median_ms"], b["median_ms"], b["min_ms"], b["max_ms"]),
              file=sys.stderr, flush=True)
    st["copy"]["tile_GBps"] = round(raw / 1e9 / (st["copy"]["median_ms"] / 1e3), 1)
    out = {"tiles": nt, "rows": nr, "cols": nc, "tile_bytes": raw, "checks": agree, "stages": stages, "copy": st["copy"],
           "bytes_per_cell": {"lsop08_type0": round(s8.bytes_per_cell, 4), "lsop12_canonical": round(s12.bytes_per_cell, 4)}}
    for b in s8.buffers() + s12.buffers() + [values, copy_dst]:
        b.free()
    return out


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    shrink = int(argv[argv.index("--shrink") + 1]) if "--shrink" in argv else 1
    hip = _hip()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    ctx = gridfour_amd.GvrsHipContext(0)
    timer = gridfour_amd.GpuTimer(ctx)
    results = {name: run_workload(name, shrink, ctx, timer, hip) for name in WORKLOADS}
    out = {"method": "HIP events on the context's stream, %d timings per case taken in turn in one process after a warm-up call of each; "
                     "tiles from gf_synth_dem_dev as bench.py makes them" % REPS,
           "aim": "LSOP08 median <= LSOP12 median + (max - min) of the LSOP12 stage's own timings",
           "csrc_digest": hipbuild.csrc_digest(), "workloads": results}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
