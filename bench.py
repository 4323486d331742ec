#!/usr/bin/env python3
"""bench.py -- encode+decode throughput of the HIP GVRS tile codec on MI355X.

    python bench.py --gpus N --steps K --warmup W [--workload etopo1|dem1024|gebco_shard] [--dump-outputs DIR]

One "step" = one pass of the hot path over one batch of synthetic elevation tiles:
CodecHuffman.encode of every tile (all predictors tried, shortest kept) followed by
CodecHuffman.decode of every packing, inputs and outputs resident in HBM.

Workloads (BASELINE.json configs)
  etopo1      configs[2]: ETOPO1-shaped 10800x21600 int32 grid = 12,960 tiles of 120x150 per GPU
              (default: the configuration north_star's target is quoted on)
  dem1024     configs[1]: 1024 tiles of 200x200
  gebco_shard configs[3]: one eighth of the GEBCO-shaped grid = 11,664 tiles of 200x200 per GPU
  float256    configs[4](i):  4,096 tiles of 256x256 float32, --codec float (CodecFloat)
  float256_lsop configs[4](ii): the same floats as int-coded floats (scale 10), --codec lsop (LSOP12)

Multi-GPU: tiles are independent, so every rank owns a contiguous tile range of the global
grid and there is no data-path collective; per-GPU work is fixed (weak scaling).  The only
collectives are the timing barrier and the max-over-ranks of the elapsed time.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

METRIC = "encode+decode MB/s on int32 elevation tiles; bit-exact vs Java ref"
HBM_PEAK_GBPS = 8000.0        # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec

WORKLOADS = {
    #  name         rows cols tiles/GPU tiles_per_row  description
    "etopo1": (120, 150, 12960, 144, "ETOPO1-shaped 10800x21600 int32 grid, 120x150 tiles, full encode+decode roundtrip"),
    "dem1024": (200, 200, 1024, 32, "1024-tile batch, 200x200 int32 synthetic DEM, all 3 predictors + Huffman"),
    "gebco_shard": (200, 200, 11664, 432, "1/8 shard of the GEBCO_2023-shaped 43200x86400 int32 grid, 200x200 tiles"),
    # strong scaling: the WHOLE GEBCO-shaped grid (93,312 tiles, 14.9 GB of cells) cut into --gpus contiguous shares
    "gebco_full": (200, 200, 93312, 432, "GEBCO_2023-shaped 43200x86400 int32 grid, 200x200 tiles, all 93,312 tiles divided over the GPUs"),
    # "a variant with 5 % INT4_NULL_CODE ocean-mask blocks to exercise a6" (PredictorModelDifferencingWithNulls)
    "etopo1_nulls": (120, 150, 12960, 144, "ETOPO1-shaped grid as etopo1 with an ocean mask: 5 % of its 16x16 blocks are null "
                                           "(nearly every tile takes PredictorModelDifferencingWithNulls)"),
    # "neighbouring-cell differences mostly within +-126 with a tail into 2-3 byte codes" -- the rough surface
    # (provinces of mountains / plains / stripes, cliff and scree blocks: gf_synth_dem_style_dev): each predictor wins a share
    # of the tiles, 4-5 % of the row differences need two M32 bytes, 0.5 % three
    "etopo1_rough": (120, 150, 12960, 144, "ETOPO1-shaped grid as etopo1, rough surface: every predictor wins a share of the tiles, "
                                           "multi-byte M32 values in four tiles of five"),
    "float256": (256, 256, 4096, 64, "4096 tiles of 256x256 float32 (DEM x 0.1f), CodecFloat byte-plane stage"),
    "float256_lsop": (256, 256, 4096, 64, "4096 tiles of 256x256 float32 (DEM x 0.1f) stored as int-coded floats "
                                          "(scale 10, GvrsElementSpecificationIntCodedFloat), LSOP12"),
}
MASK_PER_MILLE = {"etopo1_nulls": 50}
STYLE = {"etopo1_rough": 1}   # GF_DEM_STYLE_ROUGH
STRONG = {"gebco_full"}       # workloads whose tile count is the whole job's (divided over the GPUs); the others are per GPU
FP64_PEAK_TFLOPS = 78.6       # MI355X vector FP64 (the roof k_lsop_predict's normal equations are priced against)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="etopo1", choices=sorted(WORKLOADS))
    ap.add_argument("--codec", default="huffman", choices=["huffman", "canon", "lsop", "float"],
                    help="huffman = CodecHuffman (the north-star path, default); canon = CodecCanonHuffman; lsop = LSOP12, canonical container; "
                         "float = CodecFloat plane split/merge (use with --workload float256)")
    ap.add_argument("--cpu-sample-tiles", type=int, default=-1, help="tiles timed on the CPU oracle (0 = skip)")
    ap.add_argument("--cpu-all-cores", action="store_true", help="(kept for old command lines: the all-cores figure is always reported now)")
    ap.add_argument("--no-verify", action="store_true", help="skip the bit-exactness checks")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64, "
                         "at most 64 MB in all: a fixed, seeded sample of the tiles where the whole batch is larger)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def _replay_is_current(rec):
    """A replayed PMC file belongs to THESE kernels only if it carries the digest of the kernel sources it was measured on
    (gridfour_amd.build.csrc_digest, written by tools/pmc_hbm.sh / pmc_issue.sh) and that digest is the tree's."""
    try:
        from gridfour_amd.build import csrc_digest
        return bool(rec.get("csrc_digest")) and rec.get("csrc_digest") == csrc_digest()
    except Exception:
        return False


# k_huffman_decode<4> is the canonical run of the fast legacy kernel (DEC_FAST_CANON): part of a CodecCanonHuffman decode
OWN_NAME = {"k_huffman_decode<4>"}


def _pmc_traffic(workload, kernel, filename="hbm_traffic.json"):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC passes (tools/pmc_hbm.sh writes
    profiles/hbm_traffic.json: FETCH_SIZE and WRITE_SIZE in separate runs, gfx950 corrections applied).
    PMC collection cannot run inside the timed process, so the per-launch figure measured for this same
    workload is REPLAYED from that file -- the returned provenance says from which commit of it; None when no
    measurement for the workload is committed.  Kernel names match exactly (template arguments stripped)."""
    here = os.path.dirname(os.path.abspath(__file__))
    path = os.path.join(here, "profiles", filename)
    try:
        rec = json.load(open(path))
    except (OSError, ValueError):
        return None, None
    if rec.get("workload") != workload:
        return None, None
    if not _replay_is_current(rec):
        # the kernels changed since tools/pmc_hbm.sh ran: no bytes are better than another kernel's bytes
        return None, "STALE: profiles/%s was measured on other kernel sources (csrc digest differs); rerun tools/pmc_hbm.sh" % filename

    def base(name):
        name = name.split("(")[0].strip()
        if name.startswith("void "):
            name = name[5:]
        if name in OWN_NAME:                            # an instantiation that belongs to another codec's launch than its siblings
            return name
        return name.split("<")[0].strip()

    by_name = {}
    for name, d in rec.get("kernels", {}).items():
        by_name[base(name)] = by_name.get(base(name), 0) + int(d["traffic"])       # instantiations of one kernel add up
    total, found = 0, False
    for part in kernel.split("+"):                      # a launch may be a pre-pass kernel + the main kernel
        if part in by_name:
            total += by_name[part]
            found = True
    if not found:
        return None, None
    commit = rec.get("commit")
    if not commit:
        try:
            import subprocess
            commit = subprocess.run(["git", "-C", here, "log", "-n", "1", "--format=%h", "--", "profiles/" + filename],
                                    capture_output=True, text=True, timeout=10).stdout.strip() or None
        except Exception:
            commit = None
    return total, "profiles/%s@%s" % (filename, commit or "unversioned")


CLOCK_HZ = 2.4e9              # MI355X_MICROARCH.md: max engine clock; 256 CUs x 4 SIMDs, ONE scalar unit per CU


def _issue_rates():
    """Measured issue costs (tools/issue_rate.hip on an MI355X, committed under profiles/): cycles per vector wave-instruction
    and SIMD -- the cheapest kind (VOP2 add) and the VOP3 / compare-select kind these kernels are mostly made of --, cycles per
    scalar-side wave-instruction (SALU or branch) and CU, all with eight waves per SIMD feeding the port."""
    here = os.path.dirname(os.path.abspath(__file__))
    import glob
    rates = {"valu_fast": 2.8, "valu_vop3": 4.26, "scalar": 1.0, "source": "defaults (no profiles/r*/issue_rate.json readable)"}
    # the newest measurement under profiles/ (directories are named r<round>_v<n>: the last one by round and number)
    def order(path):
        name = os.path.basename(os.path.dirname(path))
        nums = [int(x) for x in __import__("re").findall(r"\d+", name)] or [0]
        return nums
    found = sorted(glob.glob(os.path.join(here, "profiles", "r*", "issue_rate.json")), key=order)
    src = found[-1] if found else os.path.join(here, "profiles", "r04_v1", "issue_rate.json")
    try:
        rec = json.load(open(src))
        by = {k["kind"]: k["rates"][-1] for k in rec["kinds"]}
        rates = {"valu_fast": by["v_add_u32 x8 independent"]["cycles_per_vector_instr_per_simd"],
                 "valu_vop3": by["v_alignbit / v_bfe_u32 / v_lshl_or_b32 / v_mad_u32_u24"]["cycles_per_vector_instr_per_simd"],
                 "scalar": by["s_add_u32 x8 independent"]["cycles_per_scalar_instr_per_cu"],
                 "source": "%s (tools/issue_rate.hip, 8 waves per SIMD)" % os.path.relpath(src, here)}
    except (OSError, ValueError, KeyError, IndexError):
        pass
    return rates


def _issue_roofline(workload, kernel, n_tiles, launch_ms):
    """Second bound next to the HBM one: the instruction-issue floors of the dominant kernel, one per issue port.  Wave-instructions
    per tile (rocprofv3 --pmc SQ_INSTS_VALU / SQ_INSTS_SALU / SQ_INSTS_BRANCH of the SHIPPING library, tools/pmc_issue.sh ->
    profiles/issue_counts.json, replayed like the HBM traffic and refused when the kernel sources changed since) priced with the
    MEASURED issue costs of tools/issue_rate.hip:
      vector  VALU x c_v / 4 SIMDs per CU          c_v = 2.8 cycles (VOP2 add) ... 4.3 (VOP3, compare + select) per SIMD
      scalar  (SALU + branch) x c_s / 1 unit per CU  c_s = 1.0 cycle
    floor = the larger of the two at the CHEAPEST vector cost; `binding` names it.  (Round 3 priced VALU + SALU at one per cycle
    over four SIMDs: the scalar unit exists once per CU, a vector instruction costs a SIMD 2.8-4.3 cycles.)"""
    here = os.path.dirname(os.path.abspath(__file__))
    try:
        rec = json.load(open(os.path.join(here, "profiles", "issue_counts.json")))
    except (OSError, ValueError):
        return None
    if rec.get("workload") != workload:
        return None
    if not _replay_is_current(rec):
        return {"bound": "issue", "stale": True, "note": "profiles/issue_counts.json was measured on other kernel sources (csrc digest differs); "
                                                          "rerun tools/pmc_issue.sh"}
    valu = salu = branch = 0.0
    found = []
    for part in kernel.split("+"):
        for name, d in rec.get("kernels", {}).items():
            stripped = name[5:].strip() if name.startswith("void ") else name.strip()
            if (stripped if stripped in OWN_NAME else stripped.split("<")[0].strip()) == part:
                valu += d.get("insts_valu", 0.0)
                salu += d.get("insts_salu", 0.0)
                branch += d.get("insts_branch", 0.0)
                found.append(name)
    if not found:
        return None
    r = _issue_rates()
    per_cu = n_tiles / 256.0 / CLOCK_HZ * 1e3                     # tiles per CU -> ms per cycle-per-tile
    v_lo, v_hi = valu * r["valu_fast"] / 4.0 * per_cu, valu * r["valu_vop3"] / 4.0 * per_cu
    sc = (salu + branch) * r["scalar"] * per_cu
    floor_ms = max(v_lo, sc)
    return {"bound": "issue", "kernel": "+".join(found), "valu_per_tile": round(valu, 1), "salu_per_tile": round(salu, 1),
            "branch_per_tile": round(branch, 1),
            "vector_floor_ms": [round(v_lo, 4), round(v_hi, 4)], "scalar_floor_ms": round(sc, 4),
            "binding": "scalar unit" if sc >= v_lo else "vector issue", "floor_ms": round(floor_ms, 4),
            "avg_launch_ms": round(launch_ms, 4), "frac_of_issue_floor": round(floor_ms / launch_ms, 4),
            "rates": r, "counts_replayed_from": "profiles/issue_counts.json@%s" % (rec.get("commit") or "unversioned")}


def run_float(args, ctxs, rank, world, dist, torch, single_multi=False):
    """BASELINE config 5(i): CodecFloat.  The GPU stage is the five byte planes (split + delta on encode, running sums +
    merge on decode, CodecFloat.java:328-458); the Deflate stage is the host's zlib and is timed separately, on a sample,
    through the host entry points.  One step = planes-encode then planes-decode of every tile, device-resident."""
    import gridfour_amd
    from gridfour_amd import DeviceBuffer, DeviceTileBatch, GpuTimer, lib
    from gridfour_amd._lib import check
    n_rows, n_cols, n_tiles, tiles_per_row, descr = WORKLOADS[args.workload]
    cells = n_rows * n_cols
    n_shards = len(ctxs)
    total_shards = n_shards if single_multi else world
    pstride = int(lib().gf_float_planes_bytes(n_rows, n_cols))
    pstride = (pstride + 15) // 16 * 16
    shards = []                                        # one per device this process drives: (ctx, values, in, planes, out, timers)
    for g, ctx in enumerate(ctxs):
        # floats = integer DEM x 0.1f: generated on the device as int32, converted on the host once
        gen = DeviceTileBatch(ctx, n_rows, n_cols, n_tiles, slot_stride=16)
        gen.synth_dem(0x9E3779B97F4A7C15 + 5, tiles_per_row, tile0=(g if single_multi else rank) * n_tiles)
        ctx.synchronize()
        v = (gen.get_values().astype(np.float32) * np.float32(0.1)).reshape(n_tiles, cells)
        del gen
        d_in, d_planes, d_out = DeviceBuffer(ctx, v.nbytes), DeviceBuffer(ctx, n_tiles * pstride), DeviceBuffer(ctx, v.nbytes)
        d_in.upload(v)
        shards.append((ctx, v, d_in, d_planes, d_out, [GpuTimer(ctx) for _ in range(args.steps)], [GpuTimer(ctx) for _ in range(args.steps)]))
    ctx, vals, d_in, d_planes, d_out = shards[0][:5]

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        for sh in shards:
            sh[0].synchronize()

    def step(i=None):
        # every device's shard is enqueued from this thread (the launches are asynchronous), no sync in between
        for c, _, din, dpl, dout, te, td in shards:
            if i is not None:
                te[i].start()
            check(lib().gf_float_planes_encode_dev(c.handle, None, n_rows, n_cols, n_tiles, din.ptr, dpl.ptr, pstride), "enc")
            if i is not None:
                te[i].stop()
        for c, _, din, dpl, dout, te, td in shards:
            if i is not None:
                td[i].start()
            check(lib().gf_float_planes_decode_dev(c.handle, None, n_rows, n_cols, n_tiles, dpl.ptr, pstride, dout.ptr), "dec")
            if i is not None:
                td[i].stop()

    for _ in range(args.warmup):
        step()
    # the timers' events are recorded once outside the timed region: the first record of an event is slower than the rest
    for sh in shards:
        for tm in sh[5] + sh[6]:
            tm.start()
            tm.stop()
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    barrier()
    elapsed = time.perf_counter() - t0
    enc_avg = float(max(np.mean([t.elapsed_ms() for t in sh[5]]) for sh in shards))      # the slowest device
    dec_avg = float(max(np.mean([t.elapsed_ms() for t in sh[6]]) for sh in shards))
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        _dump_float(args.dump_outputs, shards, n_rows, n_cols, int(lib().gf_float_planes_bytes(n_rows, n_cols)), pstride)
    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return
    bit_exact, cpu_baseline, host_path = None, None, None
    if not args.no_verify:
        import oracle
        roundtrip_ok = True
        for sh in shards:                              # every shard's round trip
            back = sh[4].download(np.uint32, n_tiles * cells).reshape(n_tiles, cells)
            roundtrip_ok = roundtrip_ok and bool(np.array_equal(back, sh[1].view(np.uint32)))
        planes = d_planes.download(np.uint8, n_tiles * pstride).reshape(n_tiles, pstride)
        nb = int(lib().gf_float_planes_bytes(n_rows, n_cols))
        parity_ok = all(planes[t, :nb].tobytes() == bytes(oracle.float_planes_encode(n_rows, n_cols, vals[t].view(np.uint32)))
                        for t in range(0, n_tiles, max(1, n_tiles // 16)))
        bit_exact = bool(roundtrip_ok and parity_ok)
        ns = args.cpu_sample_tiles if args.cpu_sample_tiles >= 0 else min(n_tiles, 400)    # ~10 s: zlib level 9 dominates
        if ns > 0 and total_shards == 1:
            sub = vals[:ns]
            mb = sub.nbytes / 1e6
            c0 = time.perf_counter()
            packs = [oracle.codec_float_encode(0, n_rows, n_cols, x.view(np.uint32), 9) for x in sub]
            c1 = time.perf_counter()
            dec = [oracle.codec_float_decode(n_rows, n_cols, pk) for pk in packs]
            c2 = time.perf_counter()
            assert all(np.array_equal(np.asarray(d, np.uint32), x.view(np.uint32)) for d, x in zip(dec, sub))
            cpu_baseline = {"value": round(mb / (c2 - c0), 2), "unit": "MB/s", "cores": 1, "kind": "port",
                            "sample": "first %d tiles (%.0f MB): oracle CodecFloat incl. zlib level 9, 1 thread; encode %.1f, "
                                      "decode %.1f MB/s" % (ns, mb, mb / (c1 - c0), mb / (c2 - c1))}
            codec = gridfour_amd.CodecFloatHip(ctx, level=9)
            h0 = time.perf_counter()
            hp = codec.encode_floats_batch(0, n_rows, n_cols, sub)
            h1 = time.perf_counter()
            hv, hst = codec.decode_floats_batch(n_rows, n_cols, hp)
            h2 = time.perf_counter()
            host_path = {"encode_MBps": round(mb / (h1 - h0), 1), "decode_MBps": round(mb / (h2 - h1), 1),
                         "equals_oracle_packings": bool(hp == packs), "compressed_bytes_per_cell": round(sum(map(len, hp)) / (ns * cells), 4),
                         "note": "host entry points on the same sample: PCIe + GPU planes + zlib level 9 on the host's threads"}
            assert np.array_equal(hv.view(np.uint32), sub.view(np.uint32)) and (hst == 0).all()
    steps = args.steps
    raw_mb = n_tiles * cells * 4 / 1e6
    plane_bytes = 4.125                              # sign bit + exponent + three mantissa bytes per cell
    alg_bytes = (4.0 + plane_bytes) * n_tiles * cells
    dom_name, dom_ms = ("k_float_planes_decode", dec_avg) if dec_avg >= enc_avg else ("k_float_planes_encode", enc_avg)
    achieved = alg_bytes / (dom_ms * 1e-3) / 1e9
    out = {
        "metric": "CodecFloat plane stage encode+decode MB/s on float32 tiles (GPU stage; Deflate on the host's zlib)",
        "value": round(raw_mb * total_shards * steps / elapsed, 1), "unit": "MB/s", "n_gpus": total_shards, "steps": steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / steps * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "u8", "data": "synthetic",
        "config": {"workload": "%s: %s" % (args.workload, descr), "tile_rows": n_rows, "tile_cols": n_cols, "tiles_per_gpu": n_tiles,
                   "codec": "CodecFloat (sign / exponent / 3 delta-coded mantissa byte planes)", "sharding": "contiguous tile ranges, no collective",
                   "processes": ("one process, %d contexts" % n_shards) if single_multi else ("one per GPU (torch.distributed launcher)" if world > 1 else "one")},
        "bit_exact": bit_exact, "encode_ms": round(enc_avg, 4), "decode_ms": round(dec_avg, 4),
        "roofline": {"bound": "hbm", "kernel": dom_name, "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": _pmc_traffic(args.workload, dom_name)[0],
                     "traffic_replayed_from": _pmc_traffic(args.workload, dom_name)[1],
                     "algorithmic_bytes_per_launch": int(alg_bytes), "avg_launch_ms": round(dom_ms, 4),
                     "roundtrip_frac": round((2 * alg_bytes) / ((enc_avg + dec_avg) * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)},
        "cpu_baseline": cpu_baseline, "host_path": host_path,
    }
    print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


class _BorrowedContext:
    """A context owned by a gf_multi, with the interface DeviceTileBatch / DeviceBuffer / GpuTimer expect."""

    def __init__(self, handle, device):
        self._h = handle
        self.device = device

    @property
    def handle(self):
        return self._h

    @property
    def stream(self):
        from gridfour_amd import lib
        return lib().gf_context_stream(self._h)

    def synchronize(self):
        from gridfour_amd import lib
        from gridfour_amd._lib import check
        check(lib().gf_context_synchronize(self._h), "gf_context_synchronize")

    def reserve(self, n_rows, n_cols, n_tiles):
        from gridfour_amd import lib
        from gridfour_amd._lib import check
        check(lib().gf_context_reserve(self._h, n_rows, n_cols, n_tiles), "gf_context_reserve")


DUMP_BYTES = 60 * 2 ** 20     # --dump-outputs: what all files together may hold (under 64 MB)
DUMP_SEED = 0x5EED            # --dump-outputs: the tile sample of a shard too large to write whole


def _dump_sample(n_tiles, tile_bytes, budget):
    """The tiles of one shard that --dump-outputs writes: all of them where they fit `budget`, else a fixed, seeded sample in
    tile order.  tile_bytes is a bound from the shapes alone, so the sample never depends on what the outputs hold."""
    k = int(max(1, min(n_tiles, budget // tile_bytes)))
    if k == n_tiles:
        return np.arange(n_tiles)
    return np.sort(np.random.default_rng(DUMP_SEED).choice(n_tiles, k, replace=False))


def _dump_save(out_dir, name, a, dtype):
    np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=dtype))


def _dump_batches(out_dir, batches):
    """--dump-outputs for the integer codecs: what a caller of encode + decode receives from the last timed step, per shard.
    For every tile the packing length, the predictor (not LSOP12: its batch entry point reports none) and both statuses; for
    the sampled tiles (`tiles`) their packings' bytes, concatenated in tile order (the lengths split them), and the decoded
    cells.  Integers as float64 (exact), bytes as float32."""
    os.makedirs(out_dir, exist_ok=True)
    n_tiles = batches[0].n_tiles
    budget = DUMP_BYTES // len(batches) - (6 * 8 * n_tiles + 8192)        # the per-tile arrays and the files' headers
    for g, b in enumerate(batches):
        pre = "shard%d_" % g if len(batches) > 1 else ""
        tiles = _dump_sample(b.n_tiles, 8 * b.cells + 4 * b.stride, budget)
        lengths = b.get_lengths()
        _dump_save(out_dir, pre + "tiles", tiles, np.float64)
        _dump_save(out_dir, pre + "lengths", lengths, np.float64)
        if b.codec != "lsop":
            _dump_save(out_dir, pre + "predictors", b.get_predictors(), np.float64)
        _dump_save(out_dir, pre + "enc_status", b.get_enc_status(), np.float64)
        _dump_save(out_dir, pre + "dec_status", b.get_dec_status(), np.float64)
        packs = [np.frombuffer(b.get_packing(int(t), min(int(lengths[t]), b.stride)), np.uint8) for t in tiles]
        _dump_save(out_dir, pre + "packings", np.concatenate(packs), np.float32)
        decoded = np.stack([b.get_decoded(int(t), 1)[0] for t in tiles]).reshape(len(tiles), b.n_rows, b.n_cols)
        _dump_save(out_dir, pre + "decoded", decoded, np.float64)


def _dump_float(out_dir, shards, n_rows, n_cols, plane_bytes, pstride):
    """--dump-outputs for CodecFloat's plane stage: per shard, for the sampled tiles (`tiles`), the byte planes the encode
    wrote (as float32) and the floats the decode gave back."""
    os.makedirs(out_dir, exist_ok=True)
    cells = n_rows * n_cols
    for g, sh in enumerate(shards):
        d_planes, d_out, n_tiles = sh[3], sh[4], len(sh[1])
        pre = "shard%d_" % g if len(shards) > 1 else ""
        tiles = _dump_sample(n_tiles, 4 * cells + 4 * plane_bytes, DUMP_BYTES // len(shards) - (8 * n_tiles + 4096))
        _dump_save(out_dir, pre + "tiles", tiles, np.float64)
        planes = np.stack([d_planes.download(np.uint8, plane_bytes, int(t) * pstride) for t in tiles])
        _dump_save(out_dir, pre + "planes", planes, np.float32)
        decoded = np.stack([d_out.download(np.float32, cells, int(t) * cells * 4) for t in tiles])
        _dump_save(out_dir, pre + "decoded", decoded.reshape(len(tiles), n_rows, n_cols), np.float32)


def _verify_shard(args, batch, n_rows, n_cols, n_tiles, with_oracle, codec=None):
    """Per shard: every status OK and every tile survives the round trip; with_oracle: sampled byte parity as well."""
    codec = codec or args.codec
    lengths = batch.get_lengths()
    ok = bool((batch.get_enc_status() == 0).all() and (batch.get_dec_status() == 0).all())
    vals = batch.get_values()
    ok = ok and bool(np.array_equal(batch.get_decoded(), vals))
    if with_oracle and ok:
        import oracle
        preds = batch.get_predictors()
        for t in list(range(0, n_tiles, max(1, n_tiles // 64)))[:64]:
            if codec == "lsop":
                ref, _ = oracle.lsop12_encode(0, n_rows, n_cols, vals[t], False)
                used = preds[t]
            else:
                ref, used = (oracle.codec_canon_encode if codec == "canon" else oracle.codec_huffman_encode)(
                    0, n_rows, n_cols, vals[t])
            if ref != batch.get_packing(t, int(lengths[t])) or used != preds[t]:
                ok = False
                break
    return ok, int(lengths.astype(np.int64).sum()), vals


def _entropy(vals, n_rows, n_cols):
    """"report the generated data's zero-order entropy and c".  Zero-order (memoryless) entropy of the row
    differences of a sample of the generated tiles, in bits per cell, next to the share of null cells: what an ideal
    order-0 coder of Differencing residuals would need, to hold against compressed_bytes_per_cell * 8."""
    t = np.asarray(vals).reshape(-1, n_rows, n_cols)
    t = t[:: max(1, len(t) // 64)][:64].astype(np.int64)
    null = t == -2 ** 31
    d = (t[:, :, 1:] - t[:, :, :-1])[~(null[:, :, 1:] | null[:, :, :-1])]
    if d.size == 0:
        return None
    _, counts = np.unique(d, return_counts=True)
    p = counts / counts.sum()
    return {"bits_per_cell": round(float(-(p * np.log2(p)).sum()), 4), "of": "row differences of 64 sampled tiles (null cells left out)",
            "null_cell_share": round(float(null.mean()), 4)}


def _m32_stats(vals, preds, n_rows, n_cols):
    """What the batch asks of the codec beyond the easy case: which predictor won how many tiles (CodecHuffman.java:100-110) and
    how many M32 bytes the row differences of a sample of tiles need (CodecM32.java:105-111: 1 byte up to 126, 2 up to 254, 3 up
    to 16,638)."""
    preds = np.asarray(preds)
    winners = {str(m): round(float((preds == m).mean()), 4) for m in (1, 2, 3, 4) if (preds == m).any()}
    t = np.asarray(vals).reshape(-1, n_rows, n_cols)
    t = t[:: max(1, len(t) // 256)][:256].astype(np.int64)
    null = t == -2 ** 31
    d = np.abs((t[:, :, 1:] - t[:, :, :-1])[~(null[:, :, 1:] | null[:, :, :-1])])
    n = max(1, d.size)
    return {"winners": winners,
            "row_difference_m32_bytes": {"1": round(float((d <= 126).sum()) / n, 4), "2": round(float(((d > 126) & (d <= 254)).sum()) / n, 4),
                                         "3+": round(float((d > 254).sum()) / n, 4), "of": "256 sampled tiles"}}


def _rough_record(args, ctx, batch, n_rows, n_cols, n_tiles, tiles_per_row, seed, headline_ms, headline_c):
    """The same grid as the ROUGH surface (--workload etopo1_rough), timed beside the headline on the same batch buffers: the
    headline's surface is the codec's easiest case (Triangle wins every tile, every M32 value is one byte).  encode / decode in
    ms per batch (HIP events, 2 warm-up + 10 timed steps), winners, M32 byte shares, and the time per PACKED byte against the
    headline's (a rougher surface packs to more bytes; what is left beyond that ratio is what the harder cases cost)."""
    from gridfour_amd import GpuTimer
    batch.synth_dem(seed, tiles_per_row, tile0=0, style=STYLE["etopo1_rough"])
    ctx.synchronize()
    reps = 10
    te, td = [GpuTimer(ctx) for _ in range(reps)], [GpuTimer(ctx) for _ in range(reps)]
    for _ in range(2):
        batch.encode(codec_index=0)
        batch.decode()
    for i in range(reps):
        te[i].start()
        batch.encode(codec_index=0)
        te[i].stop()
        td[i].start()
        batch.decode()
        td[i].stop()
    ctx.synchronize()
    enc, dec = float(np.mean([t.elapsed_ms() for t in te])), float(np.mean([t.elapsed_ms() for t in td]))
    ok, packed, vals = _verify_shard(args, batch, n_rows, n_cols, n_tiles, with_oracle=True)
    cells = n_rows * n_cols
    c = packed / float(n_tiles * cells)
    raw_mb = n_tiles * cells * 4 / 1e6
    rec = {"workload": "etopo1_rough", "encode_ms": round(enc, 4), "decode_ms": round(dec, 4), "MBps": round(raw_mb / ((enc + dec) * 1e-3), 1),
           "bit_exact": bool(ok), "bytes_per_cell": round(c, 4)}
    rec.update(_m32_stats(vals, batch.get_predictors(), n_rows, n_cols))
    # its own roofline block, as the headline's: algorithmic bytes per launch (4 + c per cell) over the slower direction's time
    algo = (4.0 + c) * n_tiles * cells
    dom_ms, dom = (enc, "encode") if enc >= dec else (dec, "decode")
    ach = algo / (dom_ms * 1e-3) / 1e9
    rec["roofline"] = {"bound": "hbm", "direction": dom, "achieved": round(ach, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                       "frac": round(ach / HBM_PEAK_GBPS, 4), "algorithmic_bytes_per_launch": int(algo), "avg_launch_ms": round(dom_ms, 4),
                       "traffic": None,
                       "note": "HIP events around the whole direction (its three / four kernels) on the context's stream"}
    names = "k_huffman_encode+k_huffman_trees+k_huffman_pack+k_huffman_pack_rare" if dom == "encode" else "k_huffman_parse_trees+k_huffman_decode"
    traffic, src = _pmc_traffic("etopo1_rough", names, "hbm_traffic_rough.json")
    rec["roofline"]["traffic"] = traffic
    rec["roofline"]["traffic_replayed_from"] = src
    he, hd = headline_ms
    rec["vs_headline"] = {"encode_ms_ratio": round(enc / he, 3), "decode_ms_ratio": round(dec / hd, 3), "packed_bytes_ratio": round(c / headline_c, 3),
                          "encode_per_packed_byte": round((enc / he) / (c / headline_c), 3),
                          "decode_per_packed_byte": round((dec / hd) / (c / headline_c), 3)}
    return rec


ENC_KERNELS = {"canon": "k_canon_encode+k_canon_trees+k_canon_pack", "lsop": "k_lsop_predict16+k_lsop_predict+k_canon_pack2",
               "huffman": "k_huffman_encode+k_huffman_trees+k_huffman_pack+k_huffman_pack_rare"}
# the decode side of the two Huffman codecs is a per-tile pre-pass kernel followed by the decode kernel: both are inside the
# HIP-event bracket and both are named, so that the rocprofv3 averages under profiles/ add up to avg_launch_ms
DEC_KERNELS = {"canon": "k_canon_parse_lengths+k_huffman_decode<4>+k_canon_decode",
               "lsop": "k_canon_parse_lengths+k_lsop_head+k_lsop_unpack2+k_lsop_unpack_m32+k_lsop_reconstruct_plane+k_lsop_reconstruct+k_lsop_reconstruct_pipe",
               "huffman": "k_huffman_parse_trees+k_huffman_decode"}
SEEDS = {"dem1024": 1, "etopo1": 2, "etopo1_nulls": 2, "etopo1_rough": 2, "gebco_shard": 3, "gebco_full": 3, "float256_lsop": 5}


def _roofline_block(algo_bytes, enc_ms, dec_ms, workload, codec, traffic_file="hbm_traffic.json"):
    """The `roofline` object of a (workload, codec): the slower direction's algorithmic bytes over its HIP-event time, its replayed
    PMC traffic (None where profiles/ holds none for this workload) and -- so that "is it bandwidth?" is a number -- the rate at
    which that traffic moved (traffic_GBps) beside the algorithmic rate (achieved)."""
    dom_ms, dom, names = (enc_ms, "encode", ENC_KERNELS[codec]) if enc_ms >= dec_ms else (dec_ms, "decode", DEC_KERNELS[codec])
    ach = algo_bytes / (dom_ms * 1e-3) / 1e9
    traffic, src = _pmc_traffic(workload, names, traffic_file)
    return {"bound": "hbm", "direction": dom, "kernel": names, "achieved": round(ach, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
            "frac": round(ach / HBM_PEAK_GBPS, 4), "algorithmic_bytes_per_launch": int(algo_bytes), "avg_launch_ms": round(dom_ms, 4),
            "traffic": traffic, "traffic_GBps": round(traffic / (dom_ms * 1e-3) / 1e9, 1) if traffic else None,
            "traffic_replayed_from": src,
            "roundtrip_frac": round((2 * algo_bytes) / ((enc_ms + dec_ms) * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)}


def _int_sub_record(args, ctx, workload, codec, reps=10):
    """Another of BASELINE.json's configurations (or another codec on the headline's grid) timed in the same run, beside the headline:
    its own batch, 2 warm-up + `reps` timed steps between HIP events on the context's stream, every tile's round trip and 64
    sampled packings against the oracle.  Compact: what the driver's record needs to see that configuration measured."""
    from gridfour_amd import DeviceTileBatch, GpuTimer
    n_rows, n_cols, n_tiles, tiles_per_row, _ = WORKLOADS[workload]
    cells = n_rows * n_cols
    b = DeviceTileBatch(ctx, n_rows, n_cols, n_tiles, slot_stride=((2 * cells + 1024) + 15) // 16 * 16, codec=codec)
    b.synth_dem(0x9E3779B97F4A7C15 + SEEDS[workload], tiles_per_row, tile0=0, mask_per_mille=MASK_PER_MILLE.get(workload, 0),
                style=STYLE.get(workload, 0))
    ctx.synchronize()
    if workload == "float256_lsop":
        f = b.get_values().astype(np.float32) * np.float32(0.1)
        b.values.upload(np.floor((f * np.float32(10.0)).astype(np.float64) + 0.5).astype(np.int32))
        del f
    te, td = [GpuTimer(ctx) for _ in range(reps)], [GpuTimer(ctx) for _ in range(reps)]
    for _ in range(2):
        b.encode(codec_index=0)
        b.decode()
    for i in range(reps):
        te[i].start()
        b.encode(codec_index=0)
        te[i].stop()
        td[i].start()
        b.decode()
        td[i].stop()
    ctx.synchronize()
    enc, dec = float(np.mean([t.elapsed_ms() for t in te])), float(np.mean([t.elapsed_ms() for t in td]))
    ok, packed, _ = _verify_shard(args, b, n_rows, n_cols, n_tiles, with_oracle=True, codec=codec)
    c = packed / float(n_tiles * cells)
    raw_mb = n_tiles * cells * 4 / 1e6
    rec = {"workload": workload, "codec": codec, "tiles": n_tiles, "tile": "%dx%d" % (n_rows, n_cols), "encode_ms": round(enc, 4),
           "decode_ms": round(dec, 4), "MBps": round(raw_mb / ((enc + dec) * 1e-3), 1), "bit_exact": bool(ok), "bytes_per_cell": round(c, 4),
           "roofline": _roofline_block((4.0 + c) * n_tiles * cells, enc, dec, workload, codec)}
    b.free()
    if codec == "lsop":
        for x in (b.residuals, b.coefs, b.scratch_status):
            x.free()
    return rec


def _float_sub_record(ctx, reps=10):
    """BASELINE config 5(i) beside the headline: CodecFloat's GPU stage (the five byte planes) on 4,096 tiles of 256x256 floats, every
    tile's round trip checked, sixteen tiles' planes against the oracle's.  The Deflate stage is the host's zlib (run_float times it
    on a sample with --codec float)."""
    import oracle
    from gridfour_amd import DeviceBuffer, DeviceTileBatch, GpuTimer, lib
    from gridfour_amd._lib import check
    n_rows, n_cols, n_tiles, tiles_per_row, _ = WORKLOADS["float256"]
    cells = n_rows * n_cols
    pstride = (int(lib().gf_float_planes_bytes(n_rows, n_cols)) + 15) // 16 * 16
    gen = DeviceTileBatch(ctx, n_rows, n_cols, n_tiles, slot_stride=16)
    gen.synth_dem(0x9E3779B97F4A7C15 + 5, tiles_per_row, tile0=0)
    ctx.synchronize()
    v = (gen.get_values().astype(np.float32) * np.float32(0.1)).reshape(n_tiles, cells)
    gen.free()
    d_in, d_planes, d_out = DeviceBuffer(ctx, v.nbytes), DeviceBuffer(ctx, n_tiles * pstride), DeviceBuffer(ctx, v.nbytes)
    d_in.upload(v)
    enc = lambda: check(lib().gf_float_planes_encode_dev(ctx.handle, None, n_rows, n_cols, n_tiles, d_in.ptr, d_planes.ptr, pstride), "enc")
    dec = lambda: check(lib().gf_float_planes_decode_dev(ctx.handle, None, n_rows, n_cols, n_tiles, d_planes.ptr, pstride, d_out.ptr), "dec")
    te, td = [GpuTimer(ctx) for _ in range(reps)], [GpuTimer(ctx) for _ in range(reps)]
    for _ in range(2):
        enc()
        dec()
    for i in range(reps):
        te[i].start()
        enc()
        te[i].stop()
        td[i].start()
        dec()
        td[i].stop()
    ctx.synchronize()
    e_ms, d_ms = float(np.mean([t.elapsed_ms() for t in te])), float(np.mean([t.elapsed_ms() for t in td]))
    back = d_out.download(np.uint32, n_tiles * cells).reshape(n_tiles, cells)
    ok = bool(np.array_equal(back, v.view(np.uint32)))
    nb = int(lib().gf_float_planes_bytes(n_rows, n_cols))
    for t in range(0, n_tiles, n_tiles // 16):
        pl = d_planes.download(np.uint8, nb, t * pstride)
        ok = ok and pl.tobytes() == bytes(oracle.float_planes_encode(n_rows, n_cols, v[t].view(np.uint32)))
    for x in (d_in, d_planes, d_out):
        x.free()
    algo = (4.0 + 4.125) * n_tiles * cells
    dom_ms, dom = (e_ms, "k_float_planes_encode") if e_ms >= d_ms else (d_ms, "k_float_planes_decode")
    ach = algo / (dom_ms * 1e-3) / 1e9
    return {"workload": "float256", "codec": "float (plane stage; Deflate on the host's zlib)", "tiles": n_tiles, "tile": "256x256",
            "encode_ms": round(e_ms, 4), "decode_ms": round(d_ms, 4), "MBps": round(n_tiles * cells * 4 / 1e6 / ((e_ms + d_ms) * 1e-3), 1),
            "bit_exact": ok, "roofline": {"bound": "hbm", "kernel": dom, "achieved": round(ach, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                          "frac": round(ach / HBM_PEAK_GBPS, 4), "algorithmic_bytes_per_launch": int(algo),
                                          "avg_launch_ms": round(dom_ms, 4), "traffic": None}}


def _compact_record(ctx, batch, n_tiles, reps=10):
    """gf_compact_dev on the headline batch: the timed encode leaves every packing at the start of its slot; SURVEY 8b(4)'s batch
    result -- offsets + one blob -- is this gather behind it.  Its time is reported beside the headline, not inside it."""
    from gridfour_amd import DeviceBuffer, GpuTimer, lib
    from gridfour_amd._lib import check
    lengths = batch.get_lengths()
    total = int(lengths.astype(np.int64).sum())
    d_off, d_blob = DeviceBuffer(ctx, (n_tiles + 1) * 8), DeviceBuffer(ctx, total + 64)
    run = lambda: check(lib().gf_compact_dev(ctx.handle, None, n_tiles, batch.slots.ptr, batch.stride, batch.lengths.ptr, d_off.ptr,
                                             d_blob.ptr, total + 64), "gf_compact_dev")
    tm = [GpuTimer(ctx) for _ in range(reps)]
    run()
    for t in tm:
        t.start()
        run()
        t.stop()
    ctx.synchronize()
    ms = float(np.mean([t.elapsed_ms() for t in tm]))
    off = d_off.download(np.uint64, n_tiles + 1)
    ok = int(off[n_tiles]) == total and bool(np.array_equal(np.diff(off).astype(np.uint32), lengths))
    blob = d_blob.download(np.uint8, total)
    for t in range(0, n_tiles, max(1, n_tiles // 32)):
        ok = ok and blob[int(off[t]):int(off[t + 1])].tobytes() == batch.get_packing(t, int(lengths[t]))
    d_off.free()
    d_blob.free()
    return {"compact_ms": round(ms, 4), "blob_bytes": total, "checked": bool(ok),
            "note": "gf_compact_dev (exclusive scan of the lengths + gather of the slots into one blob) on the headline batch; outside `value`"}


def _lsop_fp64_roofline(ctx, batch, n_rows, n_cols, n_tiles, reps):
    """k_lsop_predict against the FP64 roof: the normal equations of LsOptimalPredictor12.computeCoefficients
    (:335-342) are 91 multiply-adds + 13 adds = 195 FP64 flop per interior cell.  The kernel is launched on its own
    (gf_lsop12_predict_dev, the first half of the encode) and timed with HIP events on the context's stream."""
    from gridfour_amd import GpuTimer, lib
    from gridfour_amd._lib import check
    timers = [GpuTimer(ctx) for _ in range(reps)]

    def launch():
        check(lib().gf_lsop12_predict_dev(ctx.handle, None, n_rows, n_cols, n_tiles, batch.values.ptr, batch.residuals.ptr,
                                          batch.res_stride, batch.coefs.ptr, batch.scratch_status.ptr), "gf_lsop12_predict_dev")
    launch()
    for t in timers:
        t.start()
        launch()
        t.stop()
    ctx.synchronize()
    ms = float(np.mean([t.elapsed_ms() for t in timers]))
    interior = (n_rows - 2) * (n_cols - 4)
    flop = 195.0 * interior * n_tiles
    tf = flop / (ms * 1e-3) / 1e12
    return {"bound": "fp64-equivalent", "kernel": "k_lsop_predict16<true> (gf_lsop12_predict_dev)", "achieved": round(tf, 2), "peak": FP64_PEAK_TFLOPS,
            "unit": "TFLOP/s (FP64 flop the reference's loop would execute)", "frac": round(tf / FP64_PEAK_TFLOPS, 4),
            "flop_per_launch": int(flop), "avg_launch_ms": round(ms, 4),
            "note": "an EQUIVALENT-flop figure: LsOptimalPredictor12.computeCoefficients is 195 FP64 flop per interior cell (91 multiply-adds + "
                    "13 adds) and SURVEY 8d prices this stage against the FP64 roof -- the kernel itself executes none of them as FP64: the "
                    "normal equations run as an int8 Gram matrix on the matrix pipe (v_mfma_i32_32x32x32_i8 over two base-256 digits, "
                    "exact integers), the prediction and its rounding in FP32; only the 13x13 LU per tile is FP64"}


def _effective_cores():
    """Cores this process may actually use: the affinity mask, capped by the cgroup CPU quota (a container that shows 256
    CPUs may be allowed 16 cores' worth of time -- threads beyond that only take turns)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    for path, parse in (("/sys/fs/cgroup/cpu.max", lambda t: t.split()),
                        ("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", None)):
        try:
            txt = open(path).read().strip()
            if parse:
                quota, period = parse(txt)
            else:
                quota, period = txt, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read().strip()
            if quota not in ("max", "-1") and int(period) > 0:
                n = max(1, min(n, int(quota) // int(period)))
            break
        except (OSError, ValueError):
            continue
    return n


def _probe_java():
    """where is a JVM and a Gridfour jar?  Returns (java, jar, note); java / jar are None when missing (this
    image and the GPU boxes so far hold neither: the C port stands in, kind "port")."""
    import glob
    import shutil
    java = shutil.which("java")
    if not java:
        return None, None, "not found (no `java` on PATH)"
    pats = [os.environ.get("GRIDFOUR_JAR", ""), "/usr/share/java/*ridfour*.jar",
            os.path.expanduser("~/.m2/repository/org/gridfour/**/*ridfour*ore*.jar"),
            os.path.expanduser("~/.m2/repository/org/gridfour/**/*.jar"), os.path.join(ROOT, "*ridfour*.jar")]
    jars = [p for pat in pats if pat for p in glob.glob(pat, recursive=True)]
    if not jars:
        return java, None, "java at %s, no Gridfour jar (GRIDFOUR_JAR, /usr/share/java, ~/.m2, repo root): not timed" % java
    return java, jars[0], "java at %s, jar %s" % (java, jars[0])


def _java_reference(args, sub, n_rows, n_cols, gpu_packings=None):
    """The reference Java codec itself on the sample (tools/JavaCodecTimer.java: one thread, 20 warm-up passes, best of five), where
    a JVM and a Gridfour jar exist; else the probe's answer as a string.  With gpu_packings (tile of the sample -> its packing's
    bytes or None) the Java packings are compared with the GPU's byte for byte."""
    import subprocess
    import tempfile
    java, jar, note = _probe_java()
    if not java or not jar:
        return note
    codec = {"huffman": "huffman", "canon": "canon", "lsop": "lsop"}.get(args.codec)
    if codec is None:
        return note + ": no Java timing for codec %s" % args.codec
    ns = min(sub.shape[0], 2048)
    with tempfile.TemporaryDirectory() as tmp:
        raw, out = os.path.join(tmp, "tiles.raw"), os.path.join(tmp, "packings.out")
        np.ascontiguousarray(sub[:ns]).astype("<i4").tofile(raw)
        cmd = [java, "-Xmx4g", "-cp", jar, os.path.join(ROOT, "tools", "JavaCodecTimer.java"), raw, str(n_rows), str(n_cols),
               str(ns), codec, out]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        except (OSError, subprocess.TimeoutExpired) as e:
            return note + ": harness did not run (%s)" % e
        if r.returncode != 0:
            return note + ": harness failed rc=%d: %s" % (r.returncode, (r.stderr or r.stdout)[-300:])
        try:
            rec = json.loads(r.stdout.strip().splitlines()[-1])
        except (ValueError, IndexError):
            return note + ": harness output not understood: %s" % r.stdout[-200:]
        rec["harness"] = "tools/JavaCodecTimer.java, first %d tiles of the sample" % ns
        rec["where"] = note
        if gpu_packings is not None:
            import struct
            blob = open(out, "rb").read()
            pos, same = 0, 0
            for t in range(ns):
                (n,) = struct.unpack_from("<i", blob, pos)
                pos += 4
                jp = None if n < 0 else blob[pos:pos + n]
                pos += max(n, 0)
                same += int(jp == gpu_packings(t))
            rec["gpu_packings_identical_to_java"] = "%d of %d" % (same, ns)
        return rec


def _cpu_baseline(args, vals, n_rows, n_cols, n_tiles):
    """The oracle ("port": C restatement of the Java algorithm) on the host's cores, bounded sample of the same workload:
    one thread (the `value`: the north star's single-thread reference) and every core (native threads inside the oracle)."""
    import oracle
    cells = n_rows * n_cols
    ns = args.cpu_sample_tiles
    if ns < 0:
        budget = 1200e6 if args.codec == "huffman" else 400e6    # up to 1.2 GB of tiles: 9-20 s of CPU work on one core
        ns = min(n_tiles, max(64, int(budget / (4 * cells))))
    if ns <= 0:
        return None
    sub = vals[:ns]
    c0 = time.perf_counter()
    if args.codec == "lsop":
        out, ln = oracle.batch_lsop12_encode(0, n_rows, n_cols, sub)
    elif args.codec == "canon":
        out, ln, _ = oracle.batch_canon_encode(0, n_rows, n_cols, sub)
    else:
        out, ln, _ = oracle.batch_huffman_encode(0, n_rows, n_cols, sub)
    c1 = time.perf_counter()
    if args.codec == "lsop":
        dec = oracle.batch_lsop12_decode(n_rows, n_cols, out, ln)
    elif args.codec == "canon":
        dec = oracle.batch_canon_decode(n_rows, n_cols, out, ln)
    else:
        dec = oracle.batch_huffman_decode(n_rows, n_cols, out, ln)
    c2 = time.perf_counter()
    assert np.array_equal(dec, sub)
    del out, dec
    mb = sub.nbytes / 1e6
    res = {"value": round(mb / (c2 - c0), 2), "unit": "MB/s", "cores": 1, "kind": "port",
           "sample": "first %d tiles of the same workload (%.0f MB), oracle C restatement of the Java algorithm, 1 thread; "
                     "encode %.1f MB/s, decode %.1f MB/s" % (ns, mb, mb / (c1 - c0), mb / (c2 - c1)),
           "reference_java": _java_reference(args, sub, n_rows, n_cols, getattr(args, "_gpu_packings", None))}
    if args.codec == "huffman":
        nthr = _effective_cores()
        enc_s, dec_s = oracle.huffman_roundtrip_threads(nthr, 0, n_rows, n_cols, sub)
        res["all_cores"] = {"value": round(mb / (enc_s + dec_s), 2), "unit": "MB/s", "cores": nthr,
                            "sample": "the same %d tiles on %d native threads (pthreads in the oracle, one contiguous share of "
                                      "the tiles each) = every core this process may use (%d logical CPUs visible, affinity and "
                                      "cgroup CPU quota applied); encode %.0f MB/s, decode %.0f MB/s" % (
                                          ns, nthr, os.cpu_count() or 1, mb / enc_s, mb / dec_s)}
    return res


def _lsop_default_container(ctx_handle, vals, n_rows, n_cols, sample):
    """LsEncoder12's DEFAULT configuration (lsop/LsEncoder12.java:78, 180-216: deflateEnabled = true -- the Deflate container is built
    next to the canonical-Huffman one and the smaller is kept), which needs the host's zlib and therefore goes through the
    host-memory entry points: gf_lsop12_{encode,decode}_batch_i32 with deflate_enabled = 1 on the first `sample` tiles,
    PCIe-inclusive, checked against the oracle's default-configuration packings.  The device-resident line above times the
    canonical container alone (deflate_enabled = 0)."""
    import oracle
    from gridfour_amd import lib
    nt = min(sample, vals.shape[0])
    v = np.ascontiguousarray(vals[:nt])
    cells = v.shape[1]
    cap = nt * (int(lib().gf_lsop12_max_packing(n_rows, n_cols)) + 64)
    blob, off = np.empty(cap, np.uint8), np.zeros(nt + 1, np.uint64)
    types, st = np.zeros(nt, np.uint8), np.zeros(nt, np.int32)
    out = np.empty_like(v)
    p = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)
    best = {}
    for de in (1, 0):
        b = [1e9, 1e9]
        for i in range(2):
            t0 = time.perf_counter()
            rc = lib().gf_lsop12_encode_batch_i32(ctx_handle, 0, n_rows, n_cols, nt, p(v), de, p(blob), cap, p(off), p(types), p(st))
            t1 = time.perf_counter()
            assert rc == 0 and (st == 0).all()
            rc = lib().gf_lsop12_decode_batch_i32(ctx_handle, n_rows, n_cols, nt, p(blob), p(off), p(out), p(st))
            t2 = time.perf_counter()
            assert rc == 0 and (st == 0).all() and np.array_equal(out, v)
            b = [min(b[0], t1 - t0), min(b[1], t2 - t1)]
        gb = v.nbytes / 1e9
        rec = {"encode_GBps": round(gb / b[0], 3), "decode_GBps": round(gb / b[1], 3), "bytes_per_cell": round(int(off[nt]) / (nt * cells), 4),
               "container_types": {int(a): int(n) for a, n in zip(*np.unique(types, return_counts=True))}}
        if de:
            ok = all(blob[int(off[t]):int(off[t + 1])].tobytes() == oracle.lsop12_encode(0, n_rows, n_cols, v[t], True)[0]
                     for t in range(0, nt, max(1, nt // 16)))
            rec["equals_oracle_packings"] = bool(ok)
        best["deflate_enabled" if de else "deflate_disabled"] = rec
    best["sample_tiles"] = nt
    best["note"] = "host-memory entry points (PCIe-inclusive); deflate_enabled = the reference's default: zlib level 6 on the host's threads"
    return best


def _host_path(ctx_handle, vals, n_rows, n_cols):
    """The PCIe-inclusive rate of the host-memory entry points (pageable buffers in and out) on the same tiles; never the
    headline value, reported beside it."""
    from gridfour_amd import lib
    nt, cells = vals.shape
    cap = nt * cells * 2
    blob = np.empty(cap, np.uint8)
    off = np.zeros(nt + 1, np.uint64)
    st = np.zeros(nt, np.int32)
    out = np.empty_like(vals)
    p = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)
    best = [1e9, 1e9]
    for i in range(3):                                    # the first pass allocates the staging buffers
        t0 = time.perf_counter()
        rc = lib().gf_huffman_encode_batch_i32(ctx_handle, 0, n_rows, n_cols, nt, p(vals), p(blob), cap, p(off), None, p(st))
        t1 = time.perf_counter()
        assert rc == 0 and (st == 0).all()
        rc = lib().gf_huffman_decode_batch_i32(ctx_handle, n_rows, n_cols, nt, p(blob), p(off), p(out), p(st))
        t2 = time.perf_counter()
        assert rc == 0 and (st == 0).all()
        if i:
            best = [min(best[0], t1 - t0), min(best[1], t2 - t1)]
    assert np.array_equal(out, vals)
    gb = vals.nbytes / 1e9
    return {"encode_GBps": round(gb / best[0], 2), "decode_GBps": round(gb / best[1], 2),
            "roundtrip_GBps": round(gb / (best[0] + best[1]), 2),
            "note": "gf_huffman_*_batch_i32 on pageable host buffers: chunked, pinned staging, H2D / kernels / D2H overlapped"}


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    launcher = "WORLD_SIZE" in os.environ and world > 1
    if launcher and world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    # without a launcher --gpus N > 1 runs all N devices from THIS process through the library's multi-context entry points
    single_multi = (not launcher) and args.gpus > 1

    import torch
    import torch.distributed as dist

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (the codec has no CPU path)")
    # GF_BENCH_BACKEND=gloo / GF_BENCH_SHARE_GPU=1 are test hooks: they let several ranks / shards share the one GPU of a
    # test box to exercise the multi-GPU control flow (RCCL refuses two ranks on one device); the judged runs use neither
    backend = os.environ.get("GF_BENCH_BACKEND", "nccl")
    share = os.environ.get("GF_BENCH_SHARE_GPU", "") not in ("", "0")
    n_dev = torch.cuda.device_count()
    if backend != "nccl":
        local_rank %= n_dev
    if single_multi and not share and args.gpus > n_dev:
        raise SystemExit("--gpus %d but only %d device(s) visible" % (args.gpus, n_dev))
    torch.cuda.set_device(local_rank)
    if launcher:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)

    import gridfour_amd
    from gridfour_amd import DeviceTileBatch, GpuTimer, lib
    from gridfour_amd._lib import check

    n_rows, n_cols, n_tiles, tiles_per_row, descr = WORKLOADS[args.workload]
    if args.workload in STRONG:
        n_tiles //= args.gpus                                 # strong scaling: contiguous shares of one grid
    cells = n_rows * n_cols
    if (args.codec == "float") != (args.workload == "float256"):
        raise SystemExit("--codec float goes with --workload float256 (and only with it)")
    if args.workload == "float256_lsop" and args.codec != "lsop":
        raise SystemExit("--workload float256_lsop is the int-coded-float + LSOP12 configuration: use --codec lsop")
    if args.codec == "float":
        if single_multi:
            multi = gridfour_amd.GvrsHipMulti([0 if share else g for g in range(args.gpus)])
            fctx = [_BorrowedContext(lib().gf_multi_context(multi.handle, g), multi.devices[g]) for g in range(args.gpus)]
            return run_float(args, fctx, rank, world, dist, torch, single_multi=True)
        return run_float(args, [gridfour_amd.GvrsHipContext(local_rank)], rank, world, dist, torch)

    # ---- shards: one per GPU.  Under a launcher this process owns shard `rank`; in single-process mode it owns them all ----
    n_shards = args.gpus if single_multi else 1
    total_shards = args.gpus if single_multi else world
    multi = None
    if single_multi:
        multi = gridfour_amd.GvrsHipMulti([0 if share else g for g in range(n_shards)])
        ctxs = [_BorrowedContext(lib().gf_multi_context(multi.handle, g), multi.devices[g]) for g in range(n_shards)]
    else:
        ctxs = [gridfour_amd.GvrsHipContext(local_rank)]
    stride = ((2 * cells + 1024) + 15) // 16 * 16           # DEM packings are far below 2 B/cell
    seed = 0x9E3779B97F4A7C15 + SEEDS[args.workload]
    batches = []
    for g, ctx in enumerate(ctxs):
        b = DeviceTileBatch(ctx, n_rows, n_cols, n_tiles, slot_stride=stride, codec=args.codec)
        # shard s owns the contiguous tile range starting at s * n_tiles of the global grid (weak scaling)
        b.synth_dem(seed, tiles_per_row, tile0=(g if single_multi else rank) * n_tiles, mask_per_mille=MASK_PER_MILLE.get(args.workload, 0),
                    style=STYLE.get(args.workload, 0))
        ctx.synchronize()
        if args.workload == "float256_lsop":
            # config 5(ii): the float tiles of config 5(i) (DEM x 0.1f) as the reference stores them in an int-coded-float
            # element: i = (int) Math.floor((f - offset) * scale + 0.5), float product then double sum, with scale 10 and
            # offset 0 (GvrsElementIntCodedFloat.java:205); prepared once on the host, outside the timed region
            f = b.get_values().astype(np.float32) * np.float32(0.1)
            b.values.upload(np.floor((f * np.float32(10.0)).astype(np.float64) + 0.5).astype(np.int32))
            del f
        batches.append(b)

    # one HIP-event pair per timed step, kernel group and device, recorded on the stream the kernels run on and read only
    # after the timed region (no host sync inside it)
    t_enc = [[GpuTimer(ctx) for _ in range(args.steps)] for ctx in ctxs]
    t_dec = [[GpuTimer(ctx) for _ in range(args.steps)] for ctx in ctxs]

    def barrier():
        if launcher:
            dist.barrier()
        torch.cuda.synchronize()
        for ctx in ctxs:
            ctx.synchronize()

    if single_multi and args.codec != "huffman":
        # CodecCanonHuffman / LSOP12 from one process: every shard's kernels are enqueued on its own context's stream from this
        # thread, one device after the other (what gf_*_multi_dev do inside the library), no sync in between
        def step(i=None):
            for g, b in enumerate(batches):
                if i is not None:
                    t_enc[g][i].start()
                b.encode(codec_index=0)
                if i is not None:
                    t_enc[g][i].stop()
            for g, b in enumerate(batches):
                if i is not None:
                    t_dec[g][i].start()
                b.decode()
                if i is not None:
                    t_dec[g][i].stop()
    elif single_multi:
        import ctypes as C
        G = n_shards
        arr = lambda ptrs: (C.c_void_p * G)(*ptrs)
        nT = (C.c_size_t * G)(*([n_tiles] * G))
        a_vals, a_slots = arr([b.values.ptr for b in batches]), arr([b.slots.ptr for b in batches])
        a_len, a_pred = arr([b.lengths.ptr for b in batches]), arr([b.predictors.ptr for b in batches])
        a_est, a_dst = arr([b.enc_status.ptr for b in batches]), arr([b.dec_status.ptr for b in batches])
        a_dec = arr([b.decoded.ptr for b in batches])
        blob_bytes = (C.c_size_t * G)(*[n_tiles * b.stride for b in batches])

        def step(i=None):
            # the library enqueues every device's shard from this thread (launches are asynchronous), no sync in between
            if i is not None:
                for g in range(G):
                    t_enc[g][i].start()
            check(lib().gf_huffman_encode_batch_i32_multi_dev(multi.handle, 0, n_rows, n_cols, nT, a_vals, a_slots, batches[0].stride,
                                                              a_len, a_pred, a_est, 0xF), "encode_multi_dev")
            if i is not None:
                for g in range(G):
                    t_enc[g][i].stop()
                    t_dec[g][i].start()
            check(lib().gf_huffman_decode_batch_i32_multi_dev(multi.handle, n_rows, n_cols, nT, a_slots, blob_bytes, None,
                                                              batches[0].stride, a_len, a_dec, a_dst), "decode_multi_dev")
            if i is not None:
                for g in range(G):
                    t_dec[g][i].stop()
    else:
        def step(i=None):
            if i is not None:
                t_enc[0][i].start()
            batches[0].encode(codec_index=0)
            if i is not None:
                t_enc[0][i].stop()
                t_dec[0][i].start()
            batches[0].decode()
            if i is not None:
                t_dec[0][i].stop()

    for _ in range(args.warmup):
        step()
    # the timers' events are recorded once outside the timed region (the first record of an event is slower than the rest),
    # and Python's collector stays out of it
    for tg in t_enc + t_dec:
        for tm in tg:
            tm.start()
            tm.stop()
    import gc
    gc.collect()
    gc.disable()
    barrier()

    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    t_enqueued = time.perf_counter()
    barrier()
    elapsed = time.perf_counter() - t0
    gc.enable()
    # host time of the enqueue calls alone (launches are asynchronous: nothing in step() waits for the GPU unless a queue fills up).
    # What one Python thread needs per step to feed every device of the process; to hold against ms_per_step.
    host_enqueue_ms = (t_enqueued - t0) / args.steps * 1e3
    enc_ms = [np.mean([t.elapsed_ms() for t in tg]) for tg in t_enc]
    dec_ms = [np.mean([t.elapsed_ms() for t in tg]) for tg in t_dec]
    if launcher:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # (before anything below refills the batches' buffers)
    if args.dump_outputs and rank == 0:
        _dump_batches(args.dump_outputs, batches)

    # ---------------- verification (outside the timed region): EVERY shard, on every rank ----------------
    ok_all, packed_bytes, vals0 = True, 0, None
    if not args.no_verify:
        for g, b in enumerate(batches):
            ok, pb, vals = _verify_shard(args, b, n_rows, n_cols, n_tiles, with_oracle=(rank == 0 and g == 0))
            ok_all = ok_all and ok
            packed_bytes += pb
            if g == 0:
                vals0 = vals
    else:
        packed_bytes = sum(int(b.get_lengths().astype(np.int64).sum()) for b in batches)
    if launcher:
        flag = torch.tensor([1 if ok_all else 0], dtype=torch.int32, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)     # one failed shard anywhere fails the run
        ok_all = bool(flag.item())
    bit_exact = None if args.no_verify else ok_all
    c_per_cell = packed_bytes / float(len(batches) * n_tiles * cells)
    # which device every shard ran on (the record of an N-GPU run shows N distinct devices without RCCL introspection)
    def dev_record(shard, index):
        p = torch.cuda.get_device_properties(index)
        return {"shard": shard, "device": index, "name": p.name, "uuid": str(getattr(p, "uuid", "")),
                "gf_device_count": int(lib().gf_device_count())}
    if single_multi:
        devices = [dev_record(g, multi.devices[g]) for g in range(n_shards)]
    else:
        devices = [dev_record(rank, local_rank)]
        if launcher:
            gathered = [None] * world
            dist.all_gather_object(gathered, devices[0])
            devices = gathered

    # every shard's own averages (N > 1: a slow device shows in the record, not only in the max)
    per_shard = [{"shard": g if single_multi else rank, "encode_ms": round(float(e), 4), "decode_ms": round(float(d), 4)}
                 for g, (e, d) in enumerate(zip(enc_ms, dec_ms))]
    if launcher:
        gathered = [None] * world
        dist.all_gather_object(gathered, per_shard[0])
        per_shard = gathered
    cpu_baseline, host_path, rough, data_stats, extra = None, None, None, None, {}
    if rank == 0 and vals0 is not None:
        data_stats = _m32_stats(vals0, batches[0].get_predictors(), n_rows, n_cols)
    if rank == 0 and total_shards == 1 and not args.no_verify:
        # (the GPU's packing of sample tile t, for the byte-for-byte comparison with the reference Java codec where one exists)
        lens0, st0 = batches[0].get_lengths(), batches[0].get_enc_status()
        args._gpu_packings = lambda t: batches[0].get_packing(t, int(lens0[t])) if st0[t] == 0 else None
        cpu_baseline = _cpu_baseline(args, vals0, n_rows, n_cols, n_tiles)
        if args.codec == "huffman" and args.cpu_sample_tiles != 0:
            host_path = _host_path(ctxs[0].handle, vals0, n_rows, n_cols)
        if args.codec == "huffman" and args.workload == "etopo1" and args.cpu_sample_tiles != 0:
            # the other configurations north_star names, timed in this same run (each with its own batch, verified like the headline)
            extra["compact"] = _compact_record(ctxs[0], batches[0], n_tiles)
            # (it refills the headline batch's buffers with the rough surface)
            rough = _rough_record(args, ctxs[0], batches[0], n_rows, n_cols, n_tiles, tiles_per_row, seed,
                                  (float(np.max(enc_ms)), float(np.max(dec_ms))), c_per_cell)
            batches[0].free()
            extra["lsop"] = _int_sub_record(args, ctxs[0], "etopo1", "lsop")
            extra["canon"] = _int_sub_record(args, ctxs[0], "etopo1", "canon")
            extra["dem1024"] = _int_sub_record(args, ctxs[0], "dem1024", "huffman")
            extra["float256_lsop"] = _int_sub_record(args, ctxs[0], "float256_lsop", "lsop", reps=5)
            extra["float256"] = _float_sub_record(ctxs[0])

    if rank != 0:
        if launcher:
            dist.destroy_process_group()
        return

    steps = args.steps
    raw_mb = n_tiles * cells * 4 / 1e6
    value = raw_mb * total_shards * steps / elapsed
    enc_avg, dec_avg = float(np.max(enc_ms)), float(np.max(dec_ms))      # the slowest device (one device: its average)
    # algorithmic bytes per launch: encode reads 4 B/cell and writes c; decode reads c, writes 4
    alg_bytes = (4.0 + c_per_cell) * n_tiles * cells
    # the decode side of the two Huffman codecs is a per-tile pre-pass kernel followed by the decode kernel: both are inside
    # the HIP-event bracket and both are named, so that the rocprofv3 averages under profiles/ add up to avg_launch_ms
    enc_name, dec_name = ENC_KERNELS[args.codec], DEC_KERNELS[args.codec]
    dom_name, dom_ms = (dec_name, dec_avg) if dec_avg >= enc_avg else (enc_name, enc_avg)
    achieved = alg_bytes / (dom_ms * 1e-3) / 1e9
    traffic, traffic_from = _pmc_traffic(args.workload, dom_name)
    out = {
        "metric": METRIC,
        "value": round(value, 1),
        "unit": "MB/s",
        "n_gpus": total_shards,
        "steps": steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "strong" if args.workload in STRONG else "weak",
        "vs_baseline": None,
        "dtype": "int32",
        "data": "synthetic",
        "config": {"workload": "%s: %s" % (args.workload, descr), "tile_rows": n_rows, "tile_cols": n_cols,
                   "tiles_per_gpu": n_tiles, "codec": {"canon": "CodecCanonHuffman (Differencing/Linear/Triangle + canonical Huffman)",
                             "lsop": "LSOP12 (12-coefficient optimal predictor + canonical Huffman container)",
                             "huffman": "CodecHuffman (Differencing/Linear/Triangle + M32 + Huffman)"}[args.codec],
                   "sharding": "contiguous tile ranges, no collective",
                   "processes": "one per GPU (torch.distributed launcher)" if launcher else
                                ("one process, gf_multi_*_dev over %d contexts" % total_shards if single_multi else "one")},
        "bit_exact": bit_exact,
        "compressed_bytes_per_cell": round(c_per_cell, 4),
        "zero_order_entropy": _entropy(vals0, n_rows, n_cols) if vals0 is not None else None,
        "devices": devices,
        "encode_ms": round(enc_avg, 4),
        "decode_ms": round(dec_avg, 4),
        "per_shard_ms": per_shard,
        "host_enqueue_ms_per_step": round(host_enqueue_ms, 4),
        "encode_MBps": round(raw_mb / (enc_avg * 1e-3), 1),
        "decode_MBps": round(raw_mb / (dec_avg * 1e-3), 1),
        "roofline": {"bound": "hbm", "kernel": dom_name, "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS,
                     "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": traffic,
                     "traffic_GBps": round(traffic / (dom_ms * 1e-3) / 1e9, 1) if traffic else None,
                     "traffic_replayed_from": traffic_from, "traffic_stale": bool(traffic is None and traffic_from and traffic_from.startswith("STALE")),
                     "algorithmic_bytes_per_launch": int(alg_bytes),
                     "avg_launch_ms": round(dom_ms, 4),
                     "roundtrip_frac": round((2 * alg_bytes) / ((enc_avg + dec_avg) * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)},
        "cpu_baseline": cpu_baseline,
        "host_path": host_path,
    }
    if data_stats:
        out["config"]["data"] = data_stats
    if rough:
        out["rough"] = rough
    out.update(extra)
    out["roofline_issue"] = _issue_roofline(args.workload, dom_name, n_tiles, dom_ms)
    if args.codec == "lsop" and vals0 is not None and args.cpu_sample_tiles != 0:
        out["default_container"] = _lsop_default_container(ctxs[0].handle, vals0, n_rows, n_cols, 2048)
    if args.codec == "lsop":
        out["roofline_fp64"] = _lsop_fp64_roofline(ctxs[0], batches[0], n_rows, n_cols, n_tiles, max(3, min(steps, 10)))
    print(json.dumps(out))
    if launcher:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
