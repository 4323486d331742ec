"""Inputs shared by the interpolator's tests (tests/test_interp_shared_header.py on the CPU harness, tests/test_gpu_interp.py on the
GPU): blocks whose samples have full float32 mantissas, the fixed list of query points that takes every branch of the window rules
(gvrs/GvrsInterpolatorBSpline.java:374-484), and the glue between the model's Spec (tests/interp_ref.py), the harness'
GfInterpGeom and the library's gf_interp_spec."""
import ctypes as C
import os
import subprocess

import numpy as np

import interp_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("z", "zx", "zy", "zxx", "zxy", "zyy", "normal")

# GfInterpGeom (gridfour_amd/csrc/gvrs_interp_common.h)
GEOM = np.dtype([("grid", np.int32, 2), ("block", np.int32, 4), ("elem_type", np.int32), ("fill_i", np.int32), ("wrap", np.int32),
                 ("target", np.int32), ("spacing", np.float64, 2), ("fringe", np.float64, 4)], align=True)


def geom_of(spec):
    g = np.zeros(1, GEOM)
    g["grid"], g["block"] = (spec.n_rows_grid, spec.n_cols_grid), spec.block
    g["elem_type"], g["fill_i"], g["wrap"], g["target"] = spec.elem_type, spec.fill_i, spec.wrap, spec.target
    g["spacing"], g["fringe"] = (spec.row_spacing, spec.col_spacing), spec.row_fringe + spec.col_fringe
    return g


def build_harness(flags=("-O2", "-ffp-contract=off"), name="libinterp_harness.so"):
    src, so = os.path.join(HERE, "csrc", "interp_harness.cpp"), os.path.join(HERE, "csrc", name)
    subprocess.check_call(["g++", *flags, "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", so, src])
    L = C.CDLL(so)
    L.ih_interp_points.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 11 + [C.c_int]
    L.ih_interp_points.restype = None
    L.ih_geom_bytes.restype = C.c_size_t
    assert L.ih_geom_bytes() == GEOM.itemsize
    return L


def harness_interp(L, spec, block, rows, cols, col_spacing=None, threads=0):
    """the model's interface on the CPU harness: every output array is asked for"""
    rows, cols = np.ascontiguousarray(rows, np.float64).ravel(), np.ascontiguousarray(cols, np.float64).ravel()
    n = rows.size
    g, block = geom_of(spec), np.ascontiguousarray(block)
    cs = None if col_spacing is None else np.ascontiguousarray(col_spacing, np.float64).ravel()
    out = {k: np.full(n, 7.0) for k in FIELDS[:6]}
    out["normal"] = np.full((n, 3), 7.0)
    out["status"] = np.full(n, 99, np.int32)
    want_normal = spec.target >= R.FIRST
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    L.ih_interp_points(ptr(g), ptr(block), n, ptr(rows), ptr(cols), ptr(cs), *[ptr(out[k]) for k in FIELDS[:6]],
                       ptr(out["normal"]) if want_normal else None, ptr(out["status"]), threads)
    if not want_normal:
        out["normal"] = np.full((n, 3), np.nan)
    return out


def assert_same(got, want, what=""):
    """every field of every point, bit for bit; NaN where the model has NaN"""
    if "status" in got:
        assert np.array_equal(got["status"], want["status"]), (what, "status", np.flatnonzero(got["status"] != want["status"])[:8])
    for k in FIELDS:
        if k in got:
            assert R.same_bits(got[k], want[k]), (what, k)


def full_mantissa_f32(rng, shape):
    """float32 samples with random mantissa bits, exponents 2^-6 .. 2^6, either sign"""
    n = int(np.prod(shape))
    bits = rng.integers(0, 1 << 23, n, dtype=np.uint32) | (rng.integers(127 - 6, 127 + 7, n, dtype=np.uint32) << 23)
    bits |= rng.integers(0, 2, n, dtype=np.uint32) << 31
    return bits.view(np.float32).reshape(shape)


def random_block(rng, elem_type, shape, fill_i=0):
    """a block in the element's delivered dtype; INT and SHORT with fill cells, INT beyond 2^24 (the (float) cast rounds)"""
    if elem_type in (R.FLOAT, R.ICF):
        return full_mantissa_f32(rng, shape)
    if elem_type == R.INT:
        b = rng.integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)
    else:
        b = rng.integers(-2 ** 15, 2 ** 15, shape, dtype=np.int64).astype(np.int16)
    b[rng.random(shape) < 0.04] = fill_i
    b.reshape(-1)[5::23] = fill_i                                        # (some fill whatever the draw)
    return b


def float_specials(block):
    """NaN, -0.0, infinities, a subnormal and the largest float in a FLOAT block (a copy)"""
    b = block.copy()
    flat = b.reshape(-1)
    for k, v in enumerate((np.nan, -0.0, np.inf, -np.inf, 1e-45, 3.4028235e38, 0.0)):
        flat[(7 * k + 3) % flat.size] = np.float32(v)
    return b


def fixed_points(spec):
    """query points at every place where the window rules branch, as (rows, cols): integer coordinates, the first and last row
    and column, both sides of each fringe edge, iCol at every boundary of the standard range and of the wrapped windows (one step
    beyond what the reference's readBlock accepts included), the edges of the block, NaN and infinite coordinates"""
    n_rows, n_cols = spec.n_rows_grid, spec.n_cols_grid
    b_row0, b_col0, b_rows, b_cols = spec.block
    tiny = 2.0 ** -45
    r_mid, c_mid = b_row0 + b_rows / 2.0 + 0.25, b_col0 + b_cols / 2.0 + 0.375
    rows = [0.0, -0.0, 1.0, 2.0, n_rows - 3.0, n_rows - 2.0, n_rows - 1.0, n_rows - 1.0 - tiny, 0.5, n_rows - 1.5, n_rows - 0.75, -0.25,
            spec.row_fringe[0], np.nextafter(spec.row_fringe[0], -np.inf), np.nextafter(spec.row_fringe[0], np.inf),
            spec.row_fringe[1], np.nextafter(spec.row_fringe[1], np.inf), np.nextafter(spec.row_fringe[1], -np.inf),
            b_row0 + 0.5, b_row0 + 1.0, b_row0 + 1.5, b_row0 - 0.5, b_row0 + b_rows - 3.0, b_row0 + b_rows - 2.5, b_row0 + b_rows - 2.0,
            b_row0 + b_rows - 1.0, np.nan, np.inf, -np.inf, 1e300, -1e300, r_mid, r_mid + tiny, 3.0 - 2.0 ** -51]
    cols = [0.0, -0.0, -tiny, tiny, 0.5, 1.0, 1.0 - tiny, 1.5, 2.0, n_cols - 3.0, n_cols - 3.0 - tiny, n_cols - 2.5, n_cols - 2.0,
            n_cols - 2.0 - tiny, n_cols - 1.5, n_cols - 1.0, n_cols - 1.0 - tiny, n_cols - 0.75, n_cols + 0.0, n_cols + 0.5, n_cols + 1.0,
            n_cols + 1.5, n_cols + 2.5, -0.25, -1.0, -1.5, -2.0, -2.5, -3.0, -3.5, -4.5,
            spec.col_fringe[0], np.nextafter(spec.col_fringe[0], -np.inf), np.nextafter(spec.col_fringe[0], np.inf),
            spec.col_fringe[1], np.nextafter(spec.col_fringe[1], np.inf), np.nextafter(spec.col_fringe[1], -np.inf),
            b_col0 + 0.5, b_col0 + 1.0, b_col0 + 1.5, b_col0 - 0.5, b_col0 + b_cols - 3.0, b_col0 + b_cols - 2.5, b_col0 + b_cols - 2.0,
            b_col0 + b_cols - 1.0, np.nan, np.inf, -np.inf, 1e300, -1e300, 2147483647.5, -2147483648.5, 4294967296.5, c_mid, c_mid + tiny]
    r, c = np.array(rows), np.array(cols)
    # every row case at a middle column and at the first / last column cases; every column case at a middle row and at the edges
    pr = np.concatenate([r, np.full(c.size, r_mid), np.repeat(r, 6), np.tile([0.0, n_rows - 1.0, -0.25], c.size)])
    pc = np.concatenate([np.full(r.size, c_mid), c, np.tile([0.0, 0.5, n_cols - 1.0, n_cols - 1.5, -0.25, n_cols + 0.25], r.size),
                         np.repeat(c, 3)])
    return pr, pc


def random_points(rng, spec, n):
    """uniform over the grid and a margin that reaches beyond the fringe and the wrapped windows, a share on integer and
    half-integer coordinates"""
    rows = rng.uniform(-1.0, spec.n_rows_grid, n)
    cols = rng.uniform(-3.5, spec.n_cols_grid + 2.5, n)
    k = n // 8
    rows[:k], cols[k:2 * k] = np.round(rows[:k]), np.round(cols[k:2 * k])
    rows[2 * k:3 * k] = np.round(rows[2 * k:3 * k] * 2) / 2
    return rows, cols


def points(rng, spec, n_random):
    fr, fc = fixed_points(spec)
    rr, rc = random_points(rng, spec, n_random)
    return np.concatenate([fr, rr]), np.concatenate([fc, rc])


def lib_spec(spec):
    """the model's Spec as the library's gf_interp_spec"""
    import gridfour_amd
    return gridfour_amd.interp_spec(spec.n_rows_grid, spec.n_cols_grid, spec.block, spec.elem_type, spec.fill_i, spec.wrap, spec.target,
                                    spec.row_spacing, spec.col_spacing, spec.row_fringe, spec.col_fringe)
