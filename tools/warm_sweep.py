"""Decode time, synchronisation rounds and redone subsequences vs warm-up length of the Huffman subsequence synchronisation
(experiment; the diagnostic library's phaseLimit >> 8 hook).
usage: warm_sweep.py [warm ...]      GF_SHAPE=rows,cols,tiles,tilesPerRow (default 120,150,12960,144)  GF_DEM_STYLE=1: the rough surface
                                     GF_CODEC=huffman|canon"""
import ctypes as C, os, sys
os.environ["GVRS_HIP_DIAG"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gridfour_amd
from gridfour_amd import DeviceBuffer, DeviceTileBatch, GpuTimer, lib
ctx = gridfour_amd.GvrsHipContext(0)
n_rows, n_cols, nt, tpr = [int(x) for x in os.environ.get("GF_SHAPE", "120,150,12960,144").split(",")]
style = int(os.environ.get("GF_DEM_STYLE", "0"))
codec = os.environ.get("GF_CODEC", "huffman")
b = DeviceTileBatch(ctx, n_rows, n_cols, nt, slot_stride=(2 * n_rows * n_cols + 1024 + 15) // 16 * 16, codec=codec)
b.synth_dem(0x9E3779B97F4A7C15 + 2, tpr, style=style)
L = lib(); L.gf_internal_set_phase_limits.argtypes = [C.c_int, C.c_int]
L.gf_internal_set_decode_debug.argtypes = [C.c_void_p]
dbg = DeviceBuffer(ctx, 16 * 4 * nt).fill(0)
b.encode(); ctx.synchronize()
vals = b.get_values()
print("%dx%d, %d tiles, %s, style %d" % (n_rows, n_cols, nt, codec, style))
for warm in [int(x) for x in sys.argv[1:]] or (128, 96, 80, 64, 48, 32, 128):
    L.gf_internal_set_phase_limits(0, warm << 8)
    for _ in range(2): b.decode()
    tm = GpuTimer(ctx); tm.start()
    for _ in range(10): b.decode()
    tm.stop(); ms = tm.elapsed_ms() / 10
    ok = np.array_equal(b.get_decoded(), vals) and (b.get_dec_status() == 0).all()
    # one more decode with the per-tile record: slot 11 = rounds of the synchronisation pass, slot 9 = subsequences listed for a redo
    dbg.fill(0)
    L.gf_internal_set_decode_debug(dbg.ptr)
    b.decode(); ctx.synchronize()
    L.gf_internal_set_decode_debug(None)
    st = dbg.download(np.uint32, 16 * nt).reshape(nt, 16).astype(np.int64)
    r, ls = st[:, 11], st[:, 9]
    print("warm %3d bits: decode %.3f ms ok=%s  rounds median %d p90 %d max %d  listed/tile mean %.2f p90 %d max %d" % (
        warm, ms, ok, np.median(r), np.percentile(r, 90), r.max(), ls.mean(), np.percentile(ls, 90), ls.max()))
L.gf_internal_set_phase_limits(0, 0)
