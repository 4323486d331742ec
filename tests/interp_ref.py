"""A numpy model of the reference's B-spline interpolator over a grid block, written from the Java and independent of the C++:
gvrs/GvrsInterpolatorBSpline.java (loadSamples :374-445, loadWrappingSamples :447-484, blockLimit :307-314, zInterpGrid :327-334,
zNormalGrid :283-304) and interpolation/InterpolatorBSpline.java (interpolate :159-379), InterpolationResult.java:129-139.

Every arithmetic step is one numpy ufunc on float64 arrays -- one IEEE operation, rounded once, no fused multiply-add -- in the
order in which the Java writes it (Python's precedence and left-to-right association are Java's for these expressions).  Samples
are float32, widened to float64 before use.  All points of a call are evaluated together; integer quantities are int64 arrays that
hold Java int values (wrap32 where the Java could overflow).

Per-point status, first match (include/gvrs_hip_codec.h): ERR_ARG a NaN coordinate; DECLINED outside the fringe; ERR_ARG a wrapped
window readBlock rejects; ERR_BOUNDS a window not wholly inside the block; ERR_ARG a zero column spacing with target >= FIRST.
"""
import numpy as np

OK, DECLINED, ERR_BOUNDS, ERR_ARG = 0, 1, -2, -4
VALUE, FIRST, SECOND = 0, 1, 2
INT, SHORT, FLOAT, ICF = 0, 1, 2, 3
F8 = np.float64


class Spec:
    """gf_interp_spec; the default fringe is (-0.5, n - 0.5) per axis (GvrsFileSpecification.java:437-440 without the 4 ulp of
    the model coordinates)"""

    def __init__(self, n_rows_grid, n_cols_grid, block=None, elem_type=FLOAT, fill_i=0, wrap=0, target=VALUE, row_spacing=1.0,
                 col_spacing=1.0, row_fringe=None, col_fringe=None):
        self.n_rows_grid, self.n_cols_grid = int(n_rows_grid), int(n_cols_grid)
        self.block = tuple(int(x) for x in (block if block is not None else (0, 0, n_rows_grid, n_cols_grid)))
        self.elem_type, self.fill_i, self.wrap, self.target = int(elem_type), int(fill_i), int(wrap), int(target)
        self.row_spacing, self.col_spacing = float(row_spacing), float(col_spacing)
        self.row_fringe = tuple(float(x) for x in (row_fringe if row_fringe is not None else (-0.5, n_rows_grid - 0.5)))
        self.col_fringe = tuple(float(x) for x in (col_fringe if col_fringe is not None else (-0.5, n_cols_grid - 0.5)))


def java_int(x):
    """(int) of a double: NaN -> 0, saturating"""
    x = np.asarray(x, F8)
    y = np.where(np.isnan(x), 0.0, np.clip(x, -2147483648.0, 2147483647.0))
    return y.astype(np.int64)


def wrap32(i):
    return ((np.asarray(i, np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def block_limit(i, n):                                                   # :307-314
    return np.where(i < 0, 0, np.where(i > n - 4, n - 4, i))


def samples_f32(block, elem_type, fill_i):
    """the block as readBlock delivers it: float32; an INT / SHORT cell equal to the fill is NaN (TileElementInt.java:150-156,
    TileElementShort.java:167-173)"""
    block = np.asarray(block)
    if elem_type in (FLOAT, ICF):
        assert block.dtype == np.float32
        return block
    assert block.dtype == (np.int32 if elem_type == INT else np.int16)
    out = block.astype(np.float32)
    out[block == fill_i] = np.float32(np.nan)
    return out


def window(spec, rows, cols):
    """loadSamples: (status, row0, col0, n1, u, v) per point; columns col0 .. col0 + n1 - 1, then columns 0 .. 3 - n1"""
    p_row, p_col = np.asarray(rows, F8), np.asarray(cols, F8)
    n_rows, n_cols = spec.n_rows_grid, spec.n_cols_grid
    nan = np.isnan(p_row) | np.isnan(p_col)
    row, col = np.where(nan, 0.0, p_row), np.where(nan, 0.0, p_col)
    status = np.zeros(row.shape, np.int32)
    # :382-392
    low, high = row < 0, row > n_rows - 1
    declined = (low & (row < spec.row_fringe[0])) | (high & (row > spec.row_fringe[1]))
    row = np.where(low, F8(0), np.where(high, F8(n_rows - 1), row))
    i_row, i_col = java_int(np.floor(row)), java_int(np.floor(col))
    standard = (1 <= i_col) & (i_col <= n_cols - 3)                      # :400
    row0 = block_limit(i_row - 1, n_rows)
    v = row - row0.astype(F8) - 1                                        # :404, :442, :482
    col0 = i_col - 1
    u = col - col0.astype(F8) - 1                                        # :403
    n1 = np.full(row.shape, 4, np.int64)
    rest = ~standard
    if spec.wrap:                                                        # :447-484
        n_wrap = n_cols - 1 if spec.wrap == 2 else n_cols
        col0_w = np.where(i_col <= 0, wrap32(n_wrap - 1 + i_col), i_col - 1)
        n1_w = wrap32(n_wrap - col0_w)
        n2_w = wrap32(4 - n1_w)
        rejected = rest & ((n1_w < 1) | (n2_w < 1))
        u_w = col - i_col.astype(F8)                                     # :481
        col0, n1, u = np.where(rest, col0_w, col0), np.where(rest, n1_w, n1), np.where(rest, u_w, u)
        declined_col = np.zeros(row.shape, bool)
    else:                                                                # :428-444
        declined_col = rest & ((col < spec.col_fringe[0]) | (col > spec.col_fringe[1]))
        neg, big = col < 0, col > n_cols - 1
        col_c = np.where(neg, F8(0), np.where(big, F8(n_cols - 1), col))
        i_col_c = np.where(neg, 0, np.where(big, n_cols - 1, i_col))
        col0_e = block_limit(i_col_c - 1, n_cols)
        u_e = col_c - col0_e.astype(F8) - 1
        col0, u = np.where(rest, col0_e, col0), np.where(rest, u_e, u)
        rejected = np.zeros(row.shape, bool)
    b_row0, b_col0, b_rows, b_cols = spec.block
    outside = (row0 < b_row0) | (row0 + 4 > b_row0 + b_rows) | (col0 < b_col0) | (col0 + n1 > b_col0 + b_cols)
    outside |= (n1 < 4) & ((b_col0 > 0) | (4 - n1 > b_col0 + b_cols))
    for mask, code in ((outside, ERR_BOUNDS), (rejected, ERR_ARG), (declined | declined_col, DECLINED), (nan, ERR_ARG)):
        status[mask] = code                                              # (the last assignment is the first match)
    return status, row0, col0, n1, u, v


def evaluate(z, p_u, p_v, row_spacing, column_spacing, target):
    """interpolate(1.0 + v, 1.0 + u, 4, 4, z, rowSpacing, columnSpacing, target) :192-378; z[r][c]: float64 arrays.
    Returns dict z, zx, zy, zxx, zxy, zyy (NaN where the target does not compute them, :295-300, :372-375)."""
    row, column = 1.0 + p_v, 1.0 + p_u
    u_col, v_row = np.floor(column), np.floor(row)                       # :192-195
    u, v = column - u_col, row - v_row
    col0, row0 = java_int(u_col) - 1, java_int(v_row) - 1
    n = 4
    # :214-228 (a 4 x 4 grid: n - 4 == 0)
    u = np.where(col0 < 0, column - 1.0, np.where(col0 > n - 4, column - 1.0 - F8(n - 4), u))
    v = np.where(row0 < 0, row - 1.0, np.where(row0 > n - 4, row - 1.0 - F8(n - 4), v))
    (z00, z01, z02, z03), (z10, z11, z12, z13), (z20, z21, z22, z23), (z30, z31, z32, z33) = z
    um1 = 1.0 - u                                                        # :270-274
    b0 = um1 * um1 * um1 / 6.0
    b1 = (3 * u * u * (u - 2) + 4) / 6.0
    b2 = (3 * u * (1 + u - u * u) + 1) / 6.0
    b3 = u * u * u / 6.0
    vm1 = 1.0 - v                                                        # :277-281
    p0 = vm1 * vm1 * vm1 / 6.0
    p1 = (3 * v * v * (v - 2) + 4) / 6.0
    p2 = (3 * v * (1 + v - v * v) + 1) / 6.0
    p3 = v * v * v / 6.0
    s0 = b0 * z00 + b1 * z01 + b2 * z02 + b3 * z03                       # :285-291
    s1 = b0 * z10 + b1 * z11 + b2 * z12 + b3 * z13
    s2 = b0 * z20 + b1 * z21 + b2 * z22 + b3 * z23
    s3 = b0 * z30 + b1 * z31 + b2 * z32 + b3 * z33
    nan = np.full(np.shape(s0), np.nan)
    out = dict(z=p0 * s0 + p1 * s1 + p2 * s2 + p3 * s3, zx=nan, zy=nan, zxx=nan, zxy=nan, zyy=nan, b=(b0, b1, b2, b3))
    if target == VALUE:
        return out
    cs, rs = column_spacing, row_spacing
    bu0 = -um1 * um1 / 2.0 / cs                                          # :310-313
    bu1 = (3.0 * u / 2.0 - 2.0) * u / cs
    bu2 = (0.5 - (3.0 * u / 2.0 - 1.0) * u) / cs
    bu3 = u * u / 2.0 / cs
    pv0 = -vm1 * vm1 / 2.0 / rs                                          # :316-319
    pv1 = (3.0 * v / 2.0 - 2.0) * v / rs
    pv2 = (0.5 - (3.0 * v / 2.0 - 1.0) * v) / rs
    pv3 = v * v / 2.0 / rs
    s0 = bu0 * z00 + bu1 * z01 + bu2 * z02 + bu3 * z03                   # :324-328
    s1 = bu0 * z10 + bu1 * z11 + bu2 * z12 + bu3 * z13
    s2 = bu0 * z20 + bu1 * z21 + bu2 * z22 + bu3 * z23
    s3 = bu0 * z30 + bu1 * z31 + bu2 * z32 + bu3 * z33
    out["zx"] = p0 * s0 + p1 * s1 + p2 * s2 + p3 * s3
    t0 = pv0 * z00 + pv1 * z10 + pv2 * z20 + pv3 * z30                   # :333-338
    t1 = pv0 * z01 + pv1 * z11 + pv2 * z21 + pv3 * z31
    t2 = pv0 * z02 + pv1 * z12 + pv2 * z22 + pv3 * z32
    t3 = pv0 * z03 + pv1 * z13 + pv2 * z23 + pv3 * z33
    out["zy"] = b0 * t0 + b1 * t1 + b2 * t2 + b3 * t3
    if target != SECOND:
        return out
    out["zxy"] = pv0 * s0 + pv1 * s1 + pv2 * s2 + pv3 * s3               # :344
    buu0 = (1 - u) / (cs * cs)                                           # :347-356
    buu1 = (3 * u - 2) / (cs * cs)
    buu2 = (1 - 3 * u) / (cs * cs)
    buu3 = u / (cs * cs)
    s0 = buu0 * z00 + buu1 * z01 + buu2 * z02 + buu3 * z03
    s1 = buu0 * z10 + buu1 * z11 + buu2 * z12 + buu3 * z13
    s2 = buu0 * z20 + buu1 * z21 + buu2 * z22 + buu3 * z23
    s3 = buu0 * z30 + buu1 * z31 + buu2 * z32 + buu3 * z33
    out["zxx"] = p0 * s0 + p1 * s1 + p2 * s2 + p3 * s3
    pvv0 = (1 - v) / (rs * rs)                                           # :358-368
    pvv1 = (3 * v - 2) / (rs * rs)
    pvv2 = (1 - 3 * v) / (rs * rs)
    pvv3 = v / (rs * rs)
    t0 = pvv0 * z00 + pvv1 * z10 + pvv2 * z20 + pvv3 * z30
    t1 = pvv0 * z01 + pvv1 * z11 + pvv2 * z21 + pvv3 * z31
    t2 = pvv0 * z02 + pvv1 * z12 + pvv2 * z22 + pvv3 * z32
    t3 = pvv0 * z03 + pvv1 * z13 + pvv2 * z23 + pvv3 * z33
    out["zyy"] = b0 * t0 + b1 * t1 + b2 * t2 + b3 * t3
    return out


def interp(spec, block, rows, cols, col_spacing=None):
    """The model of gf_block_interp_points: block is the rectangle spec.block of the raster ([n_rows, n_cols], the element's
    delivered dtype).  Returns dict z, zx, zy, zxx, zxy, zyy [n], normal [n, 3], status [n] (int32); NaN wherever the status is
    not OK and in what the target does not compute."""
    rows, cols = np.asarray(rows, F8).ravel(), np.asarray(cols, F8).ravel()
    cs = np.full(rows.shape, spec.col_spacing, F8) if col_spacing is None else np.asarray(col_spacing, F8).ravel()
    b_row0, b_col0, b_rows, b_cols = spec.block
    cells = samples_f32(np.asarray(block).reshape(b_rows, b_cols), spec.elem_type, spec.fill_i)
    with np.errstate(all="ignore"):
        status, row0, col0, n1, u, v = window(spec, rows, cols)
        if spec.target >= FIRST:
            status[(status == OK) & ((cs == 0) | (spec.row_spacing == 0))] = ERR_ARG
        ok = status == OK
        r0 = np.where(ok, row0 - b_row0, 0)
        z = []
        for r in range(4):
            line = []
            for k in range(4):
                c = np.where(k < n1, col0 + k, k - n1) - b_col0
                line.append(cells[r0 + r, np.where(ok, c, 0)].astype(F8))    # float32 widened (:231-249)
            z.append(line)
        out = evaluate(z, u, v, F8(spec.row_spacing), cs, spec.target)
        out.pop("b")
        if spec.target >= FIRST:                                         # InterpolationResult.java:129-139
            zx, zy = out["zx"], out["zy"]
            s = np.sqrt(zx * zx + zy * zy + 1)
            out["normal"] = np.stack([-zx / s, -zy / s, 1.0 / s], axis=1)
        else:
            out["normal"] = np.full((rows.size, 3), np.nan)
    for k in out:
        out[k] = np.where(ok if out[k].ndim == 1 else ok[:, None], out[k], np.nan)
    out["status"] = status
    return out


def lattice_coords(row0, col0, row_step, col_step, n_rows, n_cols):
    """point (i, j): row0 + (double)i * row_step, col0 + (double)j * col_step, one product and one sum; row-major"""
    r = F8(row0) + np.arange(n_rows, dtype=F8) * F8(row_step)
    c = F8(col0) + np.arange(n_cols, dtype=F8) * F8(col_step)
    return np.repeat(r, n_cols), np.tile(c, n_rows)


def same_bits(a, b):
    """equal bit for bit, any NaN equal to any NaN (a NaN is required, not a payload)"""
    a, b = np.asarray(a, F8), np.asarray(b, F8)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint64)[~na] == b.view(np.uint64)[~nb]).all())
