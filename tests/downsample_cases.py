"""Inputs shared by the downsampling tests (tests/test_downsample_shared_header.py on the CPU harness, tests/test_gpu_downsample.py on
the GPU): blocks of full-mantissa floats with NaN, infinities, -0.0 and subnormals among them, blocks of ints with fills at every
window position and sums that wrap, and the glue between the model (tests/downsample_ref.py) and the harness' GfDsGeom."""
import ctypes as C
import os
import subprocess

import numpy as np

import downsample_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FACTORS = (1, 2, 3, 4, 5, 8, 16, 67)
KINDS = {R.INT: "int", R.SHORT: "short", R.FLOAT: "float"}

# GfDsGeom (gridfour_amd/csrc/gvrs_downsample_common.h)
GEOM = np.dtype([("pitch", np.int64), ("out_rows", np.int64), ("out_cols", np.int64), ("row_off", np.int32), ("col_off", np.int32),
                 ("f", np.int32), ("elem_type", np.int32), ("fill_i", np.int32)], align=True)


def geom_of(block, f, elem_type, fill=0):
    r0, c0, nr, nc = R.out_rect(block, f)
    g = np.zeros(1, GEOM)
    g["pitch"], g["out_rows"], g["out_cols"] = block[3], nr, nc
    g["row_off"], g["col_off"], g["f"], g["elem_type"], g["fill_i"] = r0 * f - block[0], c0 * f - block[1], f, elem_type, fill
    return g


def build_harness(flags=("-O2", "-ffp-contract=off"), name="libdownsample_harness.so"):
    src, so = os.path.join(HERE, "csrc", "downsample_harness.cpp"), os.path.join(HERE, "csrc", name)
    subprocess.check_call(["g++", *flags, "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", so, src])
    L = C.CDLL(so)
    L.dh_downsample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.dh_downsample.restype = None
    L.dh_axis.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    L.dh_axis.restype = None
    L.dh_geom_bytes.restype = C.c_size_t
    assert L.dh_geom_bytes() == GEOM.itemsize
    return L


def harness_downsample(L, values, block, f, elem_type, fill=0, threads=0):
    """the model's interface on the CPU harness"""
    g = geom_of(block, f, elem_type, fill)
    values = np.ascontiguousarray(values, R.DTYPES[elem_type])
    assert values.size == block[2] * block[3]
    out = np.full((int(g["out_rows"][0]), int(g["out_cols"][0])), 77, R.DTYPES[elem_type])
    if out.size:
        L.dh_downsample(C.c_void_p(g.ctypes.data), C.c_void_p(values.ctypes.data), C.c_void_p(out.ctypes.data), threads)
    return out


def _window_cells(block, f):
    """(block row, block column) of cell k of the window of output cell t, as a function"""
    r0, c0, nr, nc = R.out_rect(block, f)
    ro, co = r0 * f - block[0], c0 * f - block[1]
    return nr * nc, lambda t, k: (ro + (t // nc) * f + k // f, co + (t % nc) * f + k % f)


def random_floats(rng, block, f):
    """full-mantissa float32 in +-1000; every seventh window gets a special: a NaN, +inf, -inf, both infinities, all cells -0.0,
    all cells subnormal, a subnormal among normal cells -- and -0.0 sprinkled over the rest"""
    v = rng.uniform(-1000.0, 1000.0, (block[2], block[3])).astype(np.float32)
    v[rng.random(v.shape) < 0.01] = np.float32(-0.0)
    n, cell = _window_cells(block, f)
    for t in range(0, n, 7):
        kind, k = (t // 7) % 7, (t // 7 * 5) % (f * f)
        if kind == 0:
            v[cell(t, k)] = np.nan
        elif kind in (1, 2):
            v[cell(t, k)] = np.inf if kind == 1 else -np.inf
        elif kind == 3:
            v[cell(t, 0)], v[cell(t, f * f - 1)] = np.inf, -np.inf           # (f == 1: -inf alone)
        elif kind == 4:
            for q in range(f * f):
                v[cell(t, q)] = -0.0
        elif kind == 5:
            for q in range(min(f * f, 64)):                                # (f > 8: the rest of the window stays normal)
                v[cell(t, q)] = np.float32(1e-45) * np.float32(1 + (q * 37 + t) % 1000)
        else:
            v[cell(t, k)] = np.float32(1e-40)
    return v


def random_ints(rng, block, f, elem_type, fill):
    """the upper half of the block small values (averages with every rounding case), the lower half the type's whole range (INT:
    sums that wrap); a fill in every third window, at every window position in turn; the fill value sprinkled besides"""
    dt = R.DTYPES[elem_type]
    lo, hi = (-2 ** 31, 2 ** 31) if elem_type == R.INT else (-2 ** 15, 2 ** 15)
    v = rng.integers(lo, hi, (block[2], block[3]), dtype=np.int64)
    half = block[2] // 2
    v[:half] = rng.integers(-40, 41, (half, block[3]), dtype=np.int64)
    v[v == fill] += 1                                                       # (fills only where they are put)
    v[rng.random(v.shape) < 0.2 / (f * f)] = fill
    n, cell = _window_cells(block, f)
    for t in range(0, n, 3):
        v[cell(t, (t // 3) % (f * f))] = fill
    return v.astype(dt)


def random_block(rng, block, f, elem_type, fill=0):
    return random_floats(rng, block, f) if elem_type == R.FLOAT else random_ints(rng, block, f, elem_type, fill)
