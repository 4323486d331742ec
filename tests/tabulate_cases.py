"""Inputs shared by the tabulation tests (tests/test_tabulate_shared_header.py and tests/test_tabulate_args.py on the CPU,
tests/test_gpu_tabulate.py on the GPU): the implementation's thresholds, read out of gridfour_amd/csrc/gvrs_tabulate_common.h by
text so that the cases straddle them whatever they become, the glue between the model (tests/tabulate_ref.py) and the CPU harness
(tests/csrc/tabulate_harness.cpp), and the blocks that carry the reference's traps."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import tabulate_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "gridfour_amd", "csrc", "gvrs_tabulate_common.h")


def _constants():
    text = open(HEADER).read()
    out = {}
    for name in ("GF_TAB_THREADS", "GF_TAB_MAX_GROUPS", "GF_TAB_LDS_MAX_BINS", "GF_TAB_SORT_THREADS", "GF_TAB_SORT_SHARE_MAX", "GF_TAB_SORT_SPREAD",
                 "GF_TAB_SCAN_BLOCK", "GF_TAB_RUN_BLOCK"):
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
        assert m, name
        out[name] = int(m.group(1))
    return out


CONST = _constants()
THREADS, MAX_GROUPS, LDS_MAX_BINS = CONST["GF_TAB_THREADS"], CONST["GF_TAB_MAX_GROUPS"], CONST["GF_TAB_LDS_MAX_BINS"]
SORT_THREADS, SHARE_MAX, SPREAD = CONST["GF_TAB_SORT_THREADS"], CONST["GF_TAB_SORT_SHARE_MAX"], CONST["GF_TAB_SORT_SPREAD"]
SCAN_BLOCK, RUN_BLOCK = CONST["GF_TAB_SCAN_BLOCK"], CONST["GF_TAB_RUN_BLOCK"]
REF_RANGE = (-11000, 8650, 1.0)                  # PackageData's collector: 19,652 bins


def cells_per_load(elem_type):
    return 16 // np.dtype(R.DTYPES[elem_type]).itemsize


def first_trip(elem_type):
    """cells of one workgroup's first trip through the block (whole 16-byte loads)"""
    return THREADS * cells_per_load(elem_type)


def sort_share(n):
    """gf_tab_sort_share: keys of one sort workgroup"""
    per = -(-n // SPREAD)
    return min(max(-(-per // SORT_THREADS) * SORT_THREADS, SORT_THREADS), SHARE_MAX)


def window(n_bins, def_min=0):
    """(def_min, def_max, 1.0) of a collector with n_bins counters"""
    return (def_min, def_min + n_bins - 2, 1.0)


# GfTabDenseGeom / GfTabSummary (gridfour_amd/csrc/gvrs_tabulate_common.h)
GEOM = np.dtype([("n_cells", np.int64), ("first_cell", np.int64), ("scale_used", np.float64), ("base", np.int32), ("n_counter", np.int32),
                 ("elem_type", np.int32), ("fill_i", np.int32), ("skip_fill", np.int32), ("pad", np.int32)], align=True)
SUMMARY = np.dtype([(k, np.float64 if k in ("min", "max") else np.int64) for k in R.SUMMARY_KEYS])


def build_harness(flags=("-O2", "-ffp-contract=off"), name="libtabulate_harness.so"):
    src, so = os.path.join(HERE, "csrc", "tabulate_harness.cpp"), os.path.join(HERE, "csrc", name)
    subprocess.check_call(["g++", *flags, "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", so, src])
    L = C.CDLL(so)
    L.th_java_int.argtypes, L.th_java_int.restype = [C.c_double], C.c_int32
    L.th_plan.argtypes, L.th_plan.restype = [C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p], None
    L.th_sample.argtypes, L.th_sample.restype = [C.c_double, C.c_double], C.c_int32
    L.th_sample_unit.argtypes, L.th_sample_unit.restype = [C.c_int32], C.c_int32
    L.th_index.argtypes, L.th_index.restype = [C.c_int32, C.c_int32, C.c_int32], C.c_int32
    L.th_symbol_i16.argtypes, L.th_symbol_i16.restype = [C.c_int16], C.c_uint32
    L.th_symbol_i32.argtypes, L.th_symbol_i32.restype = [C.c_int32], C.c_uint32
    L.th_dense.argtypes, L.th_dense.restype = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int], None
    L.th_geom_bytes.restype = L.th_summary_bytes.restype = C.c_size_t
    assert L.th_geom_bytes() == GEOM.itemsize and L.th_summary_bytes() == SUMMARY.itemsize
    return L


def harness_plan(L, def_min, def_max, scale):
    nc, base, su = C.c_int32(), C.c_int32(), C.c_double()
    L.th_plan(def_min, def_max, scale, C.addressof(nc), C.addressof(base), C.addressof(su))
    return dict(n_counter=nc.value, base=base.value, n_bins=nc.value + 1, scale_used=su.value)


def summary_dict(a):
    return {k: a[k][0].item() for k in R.SUMMARY_KEYS}


def harness_dense(L, values, elem_type, def_min, def_max, scale, fill_i=0, skip_fill=False, first_cell=0, into=None, threads=0):
    """the model's interface on the CPU harness"""
    p = R.plan(def_min, def_max, scale)
    v = np.ascontiguousarray(values, R.DTYPES[elem_type]).ravel()
    g = np.zeros(1, GEOM)
    g["n_cells"], g["first_cell"], g["scale_used"], g["base"], g["n_counter"] = v.size, first_cell, p["scale_used"], p["base"], p["n_counter"]
    g["elem_type"], g["fill_i"], g["skip_fill"] = elem_type, fill_i, int(bool(skip_fill) and elem_type != R.FLOAT)
    counter, s = np.full(p["n_bins"], 77, np.int32), np.zeros(1, SUMMARY)
    if into is not None:
        counter = into[0].copy()
        for k in R.SUMMARY_KEYS:
            s[k] = into[1][k]
    keep = v if v.size else np.zeros(1, v.dtype)
    L.th_dense(g.ctypes.data, keep.ctypes.data, counter.ctypes.data, s.ctypes.data, int(into is not None), threads)
    return counter, summary_dict(s)


# ---------------------------------------------------------------- blocks with the reference's traps in them

def scale_trap_block(n=4096):
    """INT samples that are multiples of 5: at scale 0.9 and 0.7 the odd ones, at 0.35 the odd multiples of 10 have a product that
    ends in .5, and the float the constructor keeps bins some of them differently than the double would (5 * 0.9f + 0.5 =
    4.99999988 -> 4, 5 * 0.9 + 0.5 = 5.0 -> 5)"""
    return (5 * (np.arange(n, dtype=np.int64) + 1)).astype(np.int32)


def float_edge_block():
    """FLOAT samples around PackageData's window -11000 .. 8650 at scale 1: infinities, 1e20 and NaN touch no counter; the halves
    beside the window's two ends"""
    return np.array([np.inf, -np.inf, 1e20, -1e20, np.nan, 8650.4, 8650.6, -11000.4, -11000.6, 0.0, -0.0, 8651.4, 8651.6, -11001.6, 0.49, -0.51],
                    np.float32)


def zero_blocks():
    """a FLOAT block whose minimum is zero, -0.0 standing before +0.0 and after it"""
    a = np.array([3.0, -0.0, 5.0, 0.0, 1.0, np.nan, 0.0, -0.0], np.float32)
    b = np.array([3.0, 0.0, 5.0, -0.0, 1.0, np.nan, -0.0, 0.0], np.float32)
    return a, b


def dem_like(rng, n, elem_type, lo=-11000, hi=8650):
    """long runs of equal neighbours with jumps, as elevation data has them; FLOAT: with fractions and some NaN"""
    steps = rng.integers(-3, 4, n) * (rng.random(n) < 0.3)
    jumps = (rng.random(n) < 0.002) * rng.integers(-4000, 4000, n)
    v = np.clip(np.cumsum(steps + jumps) + (lo + hi) // 2, lo - 40, hi + 40)
    if elem_type == R.FLOAT:
        f = (v + rng.integers(0, 8, n) / 8.0).astype(np.float32)
        f[rng.random(n) < 0.01] = np.nan
        return f
    return v.astype(R.DTYPES[elem_type])


def int_stream(n, seed=7):
    """any 32-bit keys, cheaply: a multiplicative hash of the index"""
    i = np.arange(n, dtype=np.uint64) + np.uint64(seed)
    return ((i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(29)).astype(np.uint32)
