"""What inspecting a file image on the GPU costs beside copying it: the ETOPO1-shaped INT file image of tools/file_read_rate.py --
12,960 tile records of 120 x 150 cells written by gf_block_write_elems_dev, laid in shuffled order with a metadata record in
front of every third one behind a header record, and an extended tile directory -- walked and checksummed by gf_file_inspect_dev.
    GVRS_HIP_DIAG=1 python tools/file_inspect_rate.py [--out profiles/file_inspect_rate.json] [--tile-rows 90]
HIP events on the context's stream, 20 timings per case taken in turn in one process after every case ran once; medians, min, max:
  (copy)      a device-to-device copy of image_bytes: the yardstick -- the inspector reads those bytes once and writes almost nothing
  (sound)     gf_file_inspect_dev on the image
  (walk)      the same bytes behind a header that disables checksums: the walk alone (and the tile directory's one checksum)
  (updated)   the image after gf_file_update_assemble freed every 16th tile: free nodes and a free-space directory
  (serial)    one size word in mid-file damaged so that the walk passes an anchor: the serial walk of the second half.  No aim.
The aim, stated against what is not the code under test:  median(case) <= median(copy) + spread(copy)  (spread = max - min of the
copy in this run).  With the diagnostic flavour of the library (GVRS_HIP_DIAG=1) the sound image's time is split by kernel, from
events recorded between the launches, in a series of its own.  The values and the verdicts are written as they come out; nothing
here asserts them.  Every result is compared with gf_file_inspect's on the same bytes before anything is timed."""
import ctypes as C
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gridfour_amd  # noqa: E402
from gridfour_amd import DeviceBuffer, DeviceTileBatch, lib  # noqa: E402
from gridfour_amd._lib import check  # noqa: E402
from gridfour_amd.codec import _FILE_INSPECT_REPORT, _FILE_RECORD  # noqa: E402
import caller_stream as CS  # noqa: E402
import gvrs_file_build as FB  # noqa: E402

REPS = 20
CODECS = [1, 0, 0, 3]
IDS = ["GvrsHuffman", "GvrsDeflate", "GvrsFloat", "GvrsCanonicalHuffman"]
N_ROWS, N_COLS, TILES_ACROSS = 120, 150, 144
KERNELS = ["k_inspect_anchors", "k_inspect_walk", "k_inspect_chain", "k_inspect_list", "k_inspect_crc", "k_inspect_crc_large", "k_inspect_fold"]


def _stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "spread_ms": round(max(v) - min(v), 4),
            "reps": len(v)}


def _metadata(seed):
    rec = bytearray(FB.other_record(FB.RECORD_METADATA, 64, seed=seed))
    struct.pack_into("<I", rec, len(rec) - 4, FB.crc32c(rec[:-4]))
    return bytes(rec)


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
    want = vals.reshape(tile_rows, TILES_ACROSS, N_ROWS, N_COLS).transpose(0, 2, 1, 3).reshape(grid_shape)
    master = gridfour_amd.CodecMasterHip(codec_list=CODECS, context=ctx)
    idx, blob, off, used, st = master.write_block_dev(N_ROWS, N_COLS, grid_shape, (0, 0) + grid_shape, [want], ["int"], raw=True)
    assert not st.any() and sorted(idx.tolist()) == list(range(nt))
    records = {int(idx[t]): blob[int(off[t]):int(off[t + 1])].tobytes() for t in range(nt)}
    order = [int(t) for t in np.random.default_rng(12960).permutation(nt)]
    grid = grid_shape + (N_ROWS, N_COLS)

    def build(checksums):
        return FB.build_image(grid, [FB.element("z", "int")], records, codec_ids=IDS, checksums=checksums, order=order, extended=True,
                              between=lambda k: _metadata(k) if k % 3 == 0 else b"")[0]

    sound = build(True)
    f = gridfour_amd.GvrsFileHip(sound)
    images = {"sound": (f, sound)}
    plain = build(False)
    images["walk"] = (gridfour_amd.GvrsFileHip(plain), plain)
    u = f.update_begin()
    freed = list(range(0, nt, 16))
    updated = f.update_assemble(u, [b""] * len(freed), freed, 1_700_000_000_123, image_cap=len(sound) + (1 << 20))   # (nothing grows but the directories)
    images["updated"] = (gridfour_amd.GvrsFileHip(updated), updated)
    # the damage: a metadata record in mid-file whose size word takes the tile record behind it along -- the walk lands on a record
    # start behind that tile's anchor, the link does not close, and one lane walks the rest
    recs = f.inspect().records
    k = next(i for i in range(len(recs) // 2, len(recs)) if recs[i][2] == 1 and recs[i + 1][2] == 2)
    hurt = bytearray(sound)
    struct.pack_into("<i", hurt, recs[k][0], recs[k][1] + recs[k + 1][1])
    images["serial"] = (f, bytes(hurt))

    room = len(recs) + 64
    d_report = DeviceBuffer(ctx, _FILE_INSPECT_REPORT.itemsize)
    d_bad = DeviceBuffer(ctx, nt * 4)
    d_rec = DeviceBuffer(ctx, room * _FILE_RECORD.itemsize)
    dev = {name: DeviceBuffer(ctx, len(image) + 64).fill(0).upload(np.frombuffer(image, np.uint8)) for name, (_, image) in images.items()}
    d_copy = DeviceBuffer(ctx, len(sound) + 64)
    S = CS.Stream(ctx.stream)

    def inspect(name):
        g, image = images[name]
        check(L.gf_file_inspect_dev(ctx.handle, g._h, dev[name].ptr, len(image), room, d_report.ptr, d_bad.ptr, nt, d_rec.ptr), "gf_file_inspect_dev")

    facts = {}
    for name, (g, image) in images.items():                       # every case once outside the timings, and the results checked
        inspect(name)
        ctx.synchronize()
        got = gridfour_amd.GvrsInspection(d_report.download(np.uint8, _FILE_INSPECT_REPORT.itemsize).view(_FILE_INSPECT_REPORT)[0],
                                          d_bad.download(np.int32, nt), nt, d_rec.download(np.uint8, room * _FILE_RECORD.itemsize).view(_FILE_RECORD), room)
        host = g.inspect(image)
        assert got.report() == host.report() and got.bad_tiles == host.bad_tiles and got.records == host.records, name
        facts[name] = {"image_bytes": len(image), "n_records": got.n_records, "n_by_type": got.n_by_type, "failed": got.failed, "complete": got.complete,
                       "stop": got.stop_name, "n_checksum_failures": got.n_checksum_failures}
    S.copy(d_copy.ptr, dev["sound"].ptr, len(sound))
    ctx.synchronize()
    timer = gridfour_amd.GpuTimer(ctx)
    fns = {"copy": lambda: S.copy(d_copy.ptr, dev["sound"].ptr, len(sound))}
    fns.update({name: (lambda n=name: inspect(n)) for name in images})
    ms = {k: [] for k in fns}
    for _ in range(REPS):
        for name, fn in fns.items():
            timer.start()
            fn()
            timer.stop()
            ms[name].append(timer.elapsed_ms())
    cases = {name: _stats(v) for name, v in ms.items()}
    for name, c in cases.items():
        c["GBps_of_image"] = round(facts.get(name, facts["sound"])["image_bytes"] / 1e9 / (c["median_ms"] / 1e3), 1)
    aim = cases["copy"]["median_ms"] + cases["copy"]["spread_ms"]
    conditions = {name: {"value_ms": cases[name]["median_ms"], "aim_ms": round(aim, 4), "holds": bool(cases[name]["median_ms"] <= aim)}
                  for name in ("sound", "walk", "updated")}
    split = None
    if hasattr(L, "gf_internal_inspect_time_kernels"):             # the diagnostic flavour: the split by kernel, in a series of its own
        L.gf_internal_inspect_time_kernels(1)
        per = {k: [] for k in KERNELS}
        out7 = (C.c_float * 7)()
        for _ in range(REPS):
            inspect("sound")
            assert L.gf_internal_inspect_kernel_ms(out7) == 0
            for k, v in zip(KERNELS, out7):
                per[k].append(float(v))
        L.gf_internal_inspect_time_kernels(0)
        split = {k: _stats(v) for k, v in per.items()}
    ctx.synchronize()
    seg, chunk, _ = f.inspect_plan(len(sound))
    out = {"workload": "etopo1: a file image of %d tile records of %dx%d cells in shuffled order, a metadata record in front of every third" % (nt, N_ROWS, N_COLS),
           "codec_list": CODECS, "codec_ids": IDS, "directory": "extended",
           "method": "HIP events on the context's stream, %d timings per case taken in turn in one process after one untimed run of each" % REPS,
           "csrc_digest": gridfour_amd.build.csrc_digest() if hasattr(gridfour_amd, "build") else None,
           "segment_bytes": seg, "crc_chunk_bytes": chunk, "images": facts, "cases": cases, "aim": "median <= median(copy) + spread(copy)",
           "conditions": conditions, "serial_walk": "reported, no aim", "split_by_kernel_sound": split}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
