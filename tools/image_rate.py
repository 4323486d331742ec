"""What the image calls cost on a device-resident picture: the ETOPO1-shaped image, 10,800 x 21,600 ARGB words.
    python tools/image_rate.py [--out profiles/image_rate.json] [--shrink K]
HIP events on the context's stream, REPS timings per case taken in turn in one process after a warm-up call of each; medians, min
and max.  Before the timings every output is compared bit for bit with the numpy model (tests/image_ref.py).
  split / join       gf_image_split_dev / gf_image_join_dev, both models, INT and SHORT planes; `copy` beside each: a
                     hipMemcpyAsync device-to-device that moves the same total of bytes read plus written (it reads AND writes
                     what it copies, so it copies half that total)
  reduce             gf_image_reduce_dev for f = 2, 4, 8, 60; `downsample_int` beside each: gf_block_downsample_elems_dev on the
                     same words taken as an INT block of the same shape and factor
  write / read       gf_image_write_dev (n_old == 0) and gf_image_read_dev for the whole picture in tiles of 90 x 120 as Y, Co, Cg
                     SHORT elements under the list (CodecHuffman, CodecCanonHuffman); `separately` beside each: gf_image_split_dev +
                     gf_block_write_elems_dev, gf_block_read_elems_dev + gf_image_join_dev, the caller holding the planes
aim: a case's median within its yardstick's median * (1 + the yardstick's own (max - min) / median + 1/5).  No threshold is
enforced: the numbers are written as they come out, with the verdict beside them.  --shrink K divides both sides by K."""
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
from gridfour_amd.codec import _ELEM_RANGE, _ELEM_SPEC  # noqa: E402
import image_ref as M  # noqa: E402

REPS, RECORD_REPS = 20, 7
FACTORS = (2, 4, 8, 60)
TILE = (90, 120)
NAMES = {(M.RGB, M.INT): "rgb_int", (M.RGB, M.SHORT): "rgb_short", (M.YCOCG, M.INT): "ycocg_int", (M.YCOCG, M.SHORT): "ycocg_short"}


def _hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("libamdhip64 not loadable")


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _stats(v):
    med = float(np.median(v))
    return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v)}


def _verdict(case, yard):
    """the aim: within the yardstick's own run-to-run spread plus one fifth"""
    spread = (yard["max_ms"] - yard["min_ms"]) / yard["median_ms"]
    limit = yard["median_ms"] * (1.0 + spread + 0.2)
    return {"ratio_to_yardstick": round(case["median_ms"] / yard["median_ms"], 3), "yardstick_spread": round(spread, 3),
            "limit_ms": round(limit, 4), "within_aim": bool(case["median_ms"] <= limit)}


def _picture(n_rows, n_cols):
    """a smooth picture with a little texture and varying alpha: its planes pack, as a rendered relief's do"""
    r = np.arange(n_rows, dtype=np.uint32)[:, None]
    c = np.arange(n_cols, dtype=np.uint32)[None, :]
    tex = ((r * np.uint32(7919)) ^ (c * np.uint32(104729))) >> np.uint32(5) & np.uint32(1)
    pic = (((r // 40 + c // 90 + tex) & np.uint32(0xff)) << np.uint32(16)) | (((r // 55 + c // 70 + 40 + tex) & np.uint32(0xff)) << np.uint32(8))
    pic |= (c // 100 + r // 64 + 90 + tex) & np.uint32(0xff)
    pic |= ((r + c) & np.uint32(0xff)) << np.uint32(24)
    return np.ascontiguousarray(pic)


def _time(timer, cases, reps):
    for fn in cases.values():                           # the warm-up: buffers of the context grow here, not in a timing
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
    n_rows, n_cols = 10800 // shrink, 21600 // shrink
    n = n_rows * n_cols
    L, hip = lib(), _hip()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    ctx = gridfour_amd.GvrsHipContext(0)
    timer = gridfour_amd.GpuTimer(ctx)
    stream = C.c_void_p(ctx.stream)
    pic = _picture(n_rows, n_cols)
    shown = pic | np.uint32(0xff000000)
    d_pic = DeviceBuffer(ctx, pic.nbytes + 16).upload(pic)
    d_words = DeviceBuffer(ctx, pic.nbytes + 16)
    d_planes = [DeviceBuffer(ctx, n * 4 + 16) for _ in range(3)]
    d_copy_src, d_copy = DeviceBuffer(ctx, 8 * n + 16).fill(0x5A), DeviceBuffer(ctx, 8 * n + 16)
    print("picture uploaded", file=sys.stderr, flush=True)
    results, agree = {}, {}

    def copy_d2d(nbytes):
        assert hip.hipMemcpyAsync(d_copy.ptr, d_copy_src.ptr, nbytes, 3, stream) == 0      # hipMemcpyDeviceToDevice

    # ---- split and join ----
    for (model, et), name in NAMES.items():
        dt, item = M.plane_dtype(et), (2 if et == M.SHORT else 4)
        ptrs = [b.ptr for b in d_planes]
        for b in d_planes + [d_words]:
            b.fill(0xA5)
        ctx.image_split_dev(model, et, n, d_pic.ptr, ptrs)
        ctx.image_join_dev(model, et, n, ptrs, d_words.ptr)
        ctx.synchronize()
        want = M.split(model, pic.reshape(-1))
        agree["split_" + name] = all(np.array_equal(b.download(dt, n), w.astype(dt)) for b, w in zip(d_planes, want))
        agree["join_" + name] = bool(np.array_equal(d_words.download(np.uint32, n), shown.reshape(-1)))
        del want
        moved = (4 + 3 * item) * n                       # bytes read plus written, by the split and by the join alike

        def copy():
            copy_d2d(moved // 2)

        r = _time(timer, {"split": lambda: ctx.image_split_dev(model, et, n, d_pic.ptr, ptrs),
                          "join": lambda: ctx.image_join_dev(model, et, n, ptrs, d_words.ptr), "copy": copy}, REPS)
        for k in ("split", "join", "copy"):
            r[k]["moved_GBps"] = round(moved / 1e9 / (r[k]["median_ms"] / 1e3), 1)
        for k in ("split", "join"):
            r[k].update(_verdict(r[k], r["copy"]))
        results[name] = r
        print("%s: split %.3f ms, join %.3f ms, copy %.3f ms" % (name, r["split"]["median_ms"], r["join"]["median_ms"], r["copy"]["median_ms"]),
              file=sys.stderr, flush=True)

    # ---- reduce ----
    spec = np.zeros(1, _ELEM_SPEC)
    spec["type"], spec["fill_i"] = M.INT, M.INT_MIN
    rect = np.array((0, 0, n_rows, n_cols), np.int32)
    one_in, one_out = (C.c_void_p * 1)(d_pic.ptr.value), (C.c_void_p * 1)(d_words.ptr.value)
    for f in FACTORS:
        w, h = ctx.image_reduce_size(n_cols, n_rows, f)
        d_words.fill(0xA5)
        ctx.image_reduce_dev(n_cols, n_rows, f, d_pic.ptr, d_words.ptr)
        ctx.synchronize()
        agree["reduce_f%d" % f] = bool(np.array_equal(d_words.download(np.int32, w * h).reshape(h, w), M.reduce(pic, f)))

        def downsample():
            check(L.gf_block_downsample_elems_dev(ctx.handle, None, _p(spec), 1, _p(rect), f, one_in, one_out), "gf_block_downsample_elems_dev")

        r = _time(timer, {"reduce": lambda: ctx.image_reduce_dev(n_cols, n_rows, f, d_pic.ptr, d_words.ptr), "downsample_int": downsample}, REPS)
        for k in r:
            r[k]["source_GBps"] = round(pic.nbytes / 1e9 / (r[k]["median_ms"] / 1e3), 1)
        r["reduce"].update(_verdict(r["reduce"], r["downsample_int"]))
        results["reduce_f%d" % f] = r
        print("reduce f = %d: %.3f ms, downsample_int %.3f ms" % (f, r["reduce"]["median_ms"], r["downsample_int"]["median_ms"]),
              file=sys.stderr, flush=True)

    # ---- the record forms: Y, Co, Cg as SHORT elements ----
    model, et, fill = M.YCOCG, M.SHORT, -32768
    codecs = np.array((1, 3), np.int32)
    specs = np.zeros(3, _ELEM_SPEC)
    specs["type"], specs["fill_i"] = et, fill
    ranges = np.zeros(3, _ELEM_RANGE)
    ranges["min_i"], ranges["max_i"] = -32768, 32767
    grid = np.array((n_rows, n_cols) + TILE, np.int32)
    n_out = -(-n_rows // TILE[0]) * -(-n_cols // TILE[1])
    cap = n_out * int(L.gf_tile_record_max_bytes_elems(_p(specs), 3, TILE[0], TILE[1]))
    d_blob, d_off = DeviceBuffer(ctx, cap + 64), DeviceBuffer(ctx, (n_out + 1) * 8 + 16)
    d_idx, d_used, d_st = DeviceBuffer(ctx, n_out * 4 + 16), DeviceBuffer(ctx, 3 * n_out + 16), DeviceBuffer(ctx, 3 * n_out * 4 + 16)
    three = (C.c_void_p * 3)(*[b.ptr.value for b in d_planes])

    def image_write():
        check(L.gf_image_write_dev(ctx.handle, _p(codecs), 2, model, et, fill, _p(grid), _p(rect), d_pic.ptr, 0, None, 0, None, 0, 1, d_blob.ptr, cap,
                                   d_off.ptr, d_idx.ptr, d_used.ptr, d_st.ptr), "gf_image_write_dev")

    def write_separately():
        ctx.image_split_dev(model, et, n, d_pic.ptr, [b.ptr for b in d_planes])
        check(L.gf_block_write_elems_dev(ctx.handle, None, _p(codecs), 2, _p(specs), _p(ranges), 3, _p(grid), _p(rect), three, 0, None, 0, None, 0, 1,
                                         d_blob.ptr, cap, d_off.ptr, d_idx.ptr, d_used.ptr, d_st.ptr), "gf_block_write_elems_dev")

    image_write()
    ctx.synchronize()
    offsets = d_off.download(np.uint64, n_out + 1)
    blob_bytes = int(offsets[-1])
    first = d_blob.download(np.uint8, blob_bytes)
    agree["write_statuses_ok"] = bool((d_st.download(np.int32, n_out) == 0).all())
    write_separately()
    ctx.synchronize()
    agree["write_equals_split_plus_block_write"] = bool(np.array_equal(d_off.download(np.uint64, n_out + 1), offsets) and
                                                        np.array_equal(d_blob.download(np.uint8, blob_bytes), first))
    del first
    r = _time(timer, {"image_write": image_write, "separately": write_separately}, RECORD_REPS)
    r["image_write"]["ratio_to_separately"] = round(r["image_write"]["median_ms"] / r["separately"]["median_ms"], 3)
    r["record_bytes"] = blob_bytes
    results["write_ycocg_short"] = r
    print("write: %.3f ms, separately %.3f ms, %d record bytes" % (r["image_write"]["median_ms"], r["separately"]["median_ms"], blob_bytes),
          file=sys.stderr, flush=True)

    image_write()                                       # (the records the reads below take)
    ctx.synchronize()

    def image_read():
        check(L.gf_image_read_dev(ctx.handle, _p(codecs), 2, model, et, fill, _p(grid), _p(rect), n_out, d_blob.ptr, blob_bytes, d_off.ptr, 1,
                                  d_words.ptr, d_st.ptr), "gf_image_read_dev")

    def read_separately():
        check(L.gf_block_read_elems_dev(ctx.handle, None, _p(codecs), 2, _p(specs), 3, _p(grid), _p(rect), n_out, d_blob.ptr, blob_bytes, d_off.ptr, 1,
                                        three, d_st.ptr), "gf_block_read_elems_dev")
        ctx.image_join_dev(model, et, n, [b.ptr for b in d_planes], d_words.ptr)

    for key, fn in (("read", image_read), ("read_separately", read_separately)):
        d_words.fill(0xA5)
        fn()
        ctx.synchronize()
        agree[key + "_gives_the_picture"] = bool(np.array_equal(d_words.download(np.uint32, n), shown.reshape(-1)) and
                                                 not d_st.download(np.int32, 3 * n_out).any())
    r = _time(timer, {"image_read": image_read, "separately": read_separately}, RECORD_REPS)
    r["image_read"]["ratio_to_separately"] = round(r["image_read"]["median_ms"] / r["separately"]["median_ms"], 3)
    results["read_ycocg_short"] = r
    print("read: %.3f ms, separately %.3f ms" % (r["image_read"]["median_ms"], r["separately"]["median_ms"]), file=sys.stderr, flush=True)

    out = {"workload": "etopo1 shape: a picture of %d x %d ARGB words; records: tiles of %d x %d, Y / Co / Cg as SHORT elements, codecs (1, 3)" %
                       (n_rows, n_cols, TILE[0], TILE[1]),
           "method": "HIP events on the context's stream, %d timings per case (%d for the record forms) taken in turn in one process after a "
                     "warm-up call of each" % (REPS, RECORD_REPS),
           "aim": "median <= yardstick median * (1 + yardstick (max - min) / median + 1/5); yardsticks: copy (split, join), "
                  "downsample_int (reduce)",
           "csrc_digest": hipbuild.csrc_digest(), "pixels": n, "outputs_equal_the_model_bit_for_bit": agree, "cases": results}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
