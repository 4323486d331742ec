// gvrs_interp_common.h -- the B-spline interpolator over a grid block, restated once for host and device: which 4 x 4 window of
// cells a query point takes (gvrs/GvrsInterpolatorBSpline.java:374-484 loadSamples / loadWrappingSamples, :307-314 blockLimit),
// how a cell reads as a sample (gvrs/TileElementInt.java:150-156, TileElementShort.java:167-173) and the bicubic evaluation
// (interpolation/InterpolatorBSpline.java:159-379, InterpolationResult.java:129-139).  Used by the kernels of gvrs_interp.hip and
// by a stand-alone CPU harness (tests/csrc/interp_harness.cpp).
//
// THE ARITHMETIC IS THE CONTRACT: every expression below keeps the reference's operands, order and association, because the
// results are compared bit for bit.  Doubles only, one rounding per operation (the build passes -ffp-contract=off; there is no
// fma() here and none may be added), plain / and sqrt.  Nothing is "simplified": 1.0 + u - floor(1.0 + u) is not u.
// Reference paths are relative to core/src/main/java/org/gridfour/.
#pragma once

#include <math.h>
#include <stdint.h>

#include "gvrs_common.h"

// per-point status values; identical to gf_status in include/gvrs_hip_codec.h (as GF_K_* in gvrs_kernels.h)
#define GF_IP_OK 0
#define GF_IP_DECLINED 1
#define GF_IP_ERR_BOUNDS (-2)
#define GF_IP_ERR_ARG (-4)

#define GF_IP_VALUE 0
#define GF_IP_FIRST 1
#define GF_IP_SECOND 2

// gf_interp_spec as the kernels take it
struct GfInterpGeom {
    int32_t nRowsGrid, nColsGrid;                   // the raster, each >= 4
    int32_t bRow0, bCol0, bRows, bCols;             // the rectangle of the raster the block holds
    int32_t elemType, fillI;                        // GF_ELEM_*: 0 INT, 1 SHORT, 2 FLOAT, 3 ICF
    int32_t wrap;                                   // 0 none, 1 geoWrapsLongitude, 2 ... and geoBracketsLongitude
    int32_t target;                                 // GF_IP_*
    double rowSpacing, colSpacing;
    double rowFringe0, rowFringe1, colFringe0, colFringe1;
};

// the window of a point: rows row0 .. row0 + 3; columns col0 .. col0 + n1 - 1 followed by columns 0 .. 3 - n1 (n1 == 4: one run)
struct GfInterpWindow {
    int32_t row0, col0, n1;
    double u, v;                                    // the parameters loadSamples leaves for interpolate(1.0 + v, 1.0 + u, ...)
};

struct GfInterpResult {
    double z, zx, zy, zxx, zxy, zyy;
    double normal[3];                               // (gf_interp_point, when asked for)
};

// Java's (int) of a double: NaN -> 0, saturating
GF_HD int32_t gf_interp_java_int(double x)
{
    if (x != x) return 0;
    if (x >= 2147483647.0) return 2147483647;
    if (x <= -2147483648.0) return (int32_t)0x80000000u;
    return (int32_t)x;
}

// GvrsInterpolatorBSpline.java:307-314
GF_HD int32_t gf_interp_block_limit(int32_t i, int32_t n)
{
    if (i < 0) return 0;
    if (i > n - 4) return n - 4;
    return i;
}

// loadSamples (:374-445) and loadWrappingSamples (:447-484), in two halves: what they do with the row depends on the row alone,
// what they do with the column on the column alone (every branch computes row0 = blockLimit(iRow - 1) and v = row - row0 - 1).
// The lattice kernel evaluates each half once per output row / column; gf_interp_window puts them together in the reference's order.
// Integer arithmetic wraps as Java's int does.
#define GF_IP_NAN (-100)                                                         // (between the halves only)

// :375-394, :402-404: GF_IP_OK, GF_IP_NAN, or GF_IP_DECLINED outside the row fringe
GF_HD int gf_interp_window_row(const GfInterpGeom &g, double pRow, int32_t &row0Out, double &v)
{
    double row = pRow;
    if (row != row) return GF_IP_NAN;
    const int32_t nRows = g.nRowsGrid;
    if (row < 0) {
        if (row < g.rowFringe0) return GF_IP_DECLINED;
        row = 0;
    } else if (row > nRows - 1) {
        if (row > g.rowFringe1) return GF_IP_DECLINED;
        row = nRows - 1;
    }
    const int32_t iRow = gf_interp_java_int(floor(row));
    const int32_t row0 = gf_interp_block_limit(iRow - 1, nRows);
    v = row - row0 - 1;
    row0Out = row0;
    return GF_IP_OK;
}

// :395-444, :447-484: GF_IP_OK, GF_IP_NAN, GF_IP_DECLINED outside the column fringe, or GF_IP_ERR_ARG for a wrapped window whose
// readBlock throws (n1 < 1 or n2 < 1, GvrsElement.java:457-460)
GF_HD int gf_interp_window_col(const GfInterpGeom &g, double pCol, int32_t &col0Out, int32_t &n1Out, double &u)
{
    double col = pCol;
    if (col != col) return GF_IP_NAN;
    const int32_t nCols = g.nColsGrid;
    int32_t iCol = gf_interp_java_int(floor(col));
    if (1 <= iCol && iCol <= nCols - 3) {                                       // standardHandlingLeft / Right (:137-138)
        const int32_t col0 = iCol - 1;
        u = col - col0 - 1;
        col0Out = col0, n1Out = 4;
        return GF_IP_OK;
    }
    if (g.wrap) {
        const int32_t nColsForWrap = g.wrap == 2 ? nCols - 1 : nCols;           // (:139-143)
        const int32_t col0 = iCol <= 0 ? (int32_t)((uint32_t)nColsForWrap - 1u + (uint32_t)iCol) : iCol - 1;
        const int32_t n1 = (int32_t)((uint32_t)nColsForWrap - (uint32_t)col0);
        const int32_t n2 = (int32_t)(4u - (uint32_t)n1);
        if (n1 < 1 || n2 < 1) return GF_IP_ERR_ARG;
        u = col - iCol;
        col0Out = col0, n1Out = n1;
        return GF_IP_OK;
    }
    if (col < g.colFringe0 || col > g.colFringe1) return GF_IP_DECLINED;
    if (col < 0) {
        col = 0;
        iCol = 0;
    } else if (col > nCols - 1) {
        col = nCols - 1;
        iCol = nCols - 1;
    }
    const int32_t col0 = gf_interp_block_limit(iCol - 1, nCols);
    u = col - col0 - 1;
    col0Out = col0, n1Out = 4;
    return GF_IP_OK;
}

// the two halves' verdicts in the reference's order: GF_IP_ERR_ARG for a NaN coordinate (interpolate throws on the NaN parameter,
// InterpolatorBSpline.java:181-183), the row fringe (:382-392) before anything the column decides
GF_HD int gf_interp_window_status(int rowStatus, int colStatus)
{
    if (rowStatus == GF_IP_NAN || colStatus == GF_IP_NAN) return GF_IP_ERR_ARG;
    return rowStatus != GF_IP_OK ? rowStatus : colStatus;
}

GF_HD int gf_interp_window(const GfInterpGeom &g, double pRow, double pCol, GfInterpWindow &w)
{
    w.row0 = w.col0 = 0, w.n1 = 4, w.u = w.v = 0;
    const int rs = gf_interp_window_row(g, pRow, w.row0, w.v);
    const int cs = gf_interp_window_col(g, pCol, w.col0, w.n1, w.u);
    return gf_interp_window_status(rs, cs);
}

// the window, both parts of a wrapped one, lies wholly inside the block
GF_HD bool gf_interp_window_in_block(const GfInterpGeom &g, int32_t row0, int32_t col0, int32_t n1)
{
    const int64_t r0 = g.bRow0, r1 = r0 + g.bRows, c0 = g.bCol0, c1 = c0 + g.bCols;
    if (row0 < r0 || (int64_t)row0 + 4 > r1) return false;
    if (col0 < c0 || (int64_t)col0 + n1 > c1) return false;
    if (n1 < 4 && (c0 > 0 || 4 - n1 > c1)) return false;
    return true;
}

// a cell as readBlock delivers it: float32, widened to double (InterpolatorBSpline.java:231-249)
GF_HD double gf_interp_sample_f32(uint32_t bits)
{
    union { uint32_t u; float f; } x;
    x.u = bits;
    return (double)x.f;
}
GF_HD double gf_interp_sample_i32(int32_t cell, int32_t fill)                   // TileElementInt.java:150-156, TileElementShort.java:167-173
{
    if (cell == fill) return gf_interp_sample_f32(0x7fc00000u);                 // Float.NaN
    return (double)(float)cell;
}

// The sixteen samples z[4 * r + k] of a window that lies inside the block, from memory the caller can read.  The cells come as
// words: four runs of four consecutive cells (one 16-byte load each where cells are 4 bytes wide: the address is 4-byte aligned,
// which gfx950 serves), or two runs per row when the window wraps; INT and SHORT cells are widened, and the fill turned into NaN,
// on their way into registers: no pass of its own.  Cell addresses are 64 bits wide.
GF_HD void gf_interp_samples(const GfInterpGeom &g, const void *block, int32_t row0, int32_t col0, int32_t n1, double *z)
{
    uint32_t q[16];
    const size_t stride = (size_t)g.bCols;
    const size_t rowAt = (size_t)(row0 - g.bRow0) * stride;
    const size_t at1 = rowAt + (size_t)(col0 - g.bCol0);                        // sample k < n1 of a row: cell at1 + k
    const size_t at2 = rowAt - (size_t)n1;                                      // sample k >= n1: column k - n1 of the grid (the block starts at column 0)
    if (g.elemType != 1 && n1 == 4) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const GfU4 c = *reinterpret_cast<const GfU4 *>(reinterpret_cast<const uint32_t *>(block) + (at1 + (size_t)r * stride));
            q[4 * r + 0] = c.x, q[4 * r + 1] = c.y, q[4 * r + 2] = c.z, q[4 * r + 3] = c.w;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const size_t at = (k < n1 ? at1 : at2) + (size_t)r * stride + (size_t)k;
                q[4 * r + k] = g.elemType != 1 ? reinterpret_cast<const uint32_t *>(block)[at]
                                               : (uint32_t)(int32_t) reinterpret_cast<const int16_t *>(block)[at];
            }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) z[i] = g.elemType >= 2 ? gf_interp_sample_f32(q[i]) : gf_interp_sample_i32((int32_t)q[i], g.fillI);
}

// One axis of interpolate(1.0 + v, 1.0 + u, 4, 4, ...) (InterpolatorBSpline.java:192-228, :270-281, :310-319, :347-361): the
// coordinate 1.0 + p, its floor, the re-derived parameter with the outer-band adjustment (a 4-wide grid: both branches leave the
// window at 0), then the basis functions b[] (b0..b3 / p0..p3), their derivatives d[] (bu / pv, target >= FIRST) and second
// derivatives dd[] (buu / pvv, target SECOND).  The column axis and the row axis are the same expressions with u, columnSpacing and
// v, rowSpacing.
struct GfInterpBasis {
    double b[4], d[4], dd[4];
};
GF_HD void gf_interp_basis(double p, double spacing, int target, GfInterpBasis &B)
{
    const double column = 1.0 + p;
    const double uCol = floor(column);
    double u = column - uCol;
    const int32_t iCol = gf_interp_java_int(uCol);
    int32_t col0 = iCol - 1;
    if (col0 < 0) {
        col0 = 0;
        u = column - 1.0;
    } else if (col0 > 4 - 4) {
        col0 = 4 - 4;
        u = column - 1.0 - col0;
    }
    const double um1 = 1.0 - u;
    B.b[0] = um1 * um1 * um1 / 6.0;
    B.b[1] = (3 * u * u * (u - 2) + 4) / 6.0;
    B.b[2] = (3 * u * (1 + u - u * u) + 1) / 6.0;
    B.b[3] = u * u * u / 6.0;
    if (target == GF_IP_VALUE) return;
    B.d[0] = -um1 * um1 / 2.0 / spacing;
    B.d[1] = (3.0 * u / 2.0 - 2.0) * u / spacing;
    B.d[2] = (0.5 - (3.0 * u / 2.0 - 1.0) * u) / spacing;
    B.d[3] = u * u / 2.0 / spacing;
    if (target != GF_IP_SECOND) return;
    B.dd[0] = (1 - u) / (spacing * spacing);
    B.dd[1] = (3 * u - 2) / (spacing * spacing);
    B.dd[2] = (1 - 3 * u) / (spacing * spacing);
    B.dd[3] = u / (spacing * spacing);
}

// The sums of interpolate (:285-291, :324-338, :344, :352-368) on the 16 samples z[4 * r + c]: bu is the column axis' basis, pv the
// row axis'.  The fields the target does not compute are NaN (:295-300, :372-375).
GF_HD void gf_interp_sums(const double *z, const GfInterpBasis &bu, const GfInterpBasis &pv, int target, GfInterpResult &res)
{
    const double z00 = z[0], z01 = z[1], z02 = z[2], z03 = z[3];
    const double z10 = z[4], z11 = z[5], z12 = z[6], z13 = z[7];
    const double z20 = z[8], z21 = z[9], z22 = z[10], z23 = z[11];
    const double z30 = z[12], z31 = z[13], z32 = z[14], z33 = z[15];
    const double b0 = bu.b[0], b1 = bu.b[1], b2 = bu.b[2], b3 = bu.b[3];
    const double p0 = pv.b[0], p1 = pv.b[1], p2 = pv.b[2], p3 = pv.b[3];

    double s0 = b0 * z00 + b1 * z01 + b2 * z02 + b3 * z03;
    double s1 = b0 * z10 + b1 * z11 + b2 * z12 + b3 * z13;
    double s2 = b0 * z20 + b1 * z21 + b2 * z22 + b3 * z23;
    double s3 = b0 * z30 + b1 * z31 + b2 * z32 + b3 * z33;

    const double qnan = gf_interp_sample_f32(0x7fc00000u);
    res.z = p0 * s0 + p1 * s1 + p2 * s2 + p3 * s3;
    res.zx = res.zy = res.zxx = res.zxy = res.zyy = qnan;
    if (target == GF_IP_VALUE) return;

    const double bu0 = bu.d[0], bu1 = bu.d[1], bu2 = bu.d[2], bu3 = bu.d[3];
    const double pv0 = pv.d[0], pv1 = pv.d[1], pv2 = pv.d[2], pv3 = pv.d[3];

    s0 = bu0 * z00 + bu1 * z01 + bu2 * z02 + bu3 * z03;
    s1 = bu0 * z10 + bu1 * z11 + bu2 * z12 + bu3 * z13;
    s2 = bu0 * z20 + bu1 * z21 + bu2 * z22 + bu3 * z23;
    s3 = bu0 * z30 + bu1 * z31 + bu2 * z32 + bu3 * z33;
    res.zx = p0 * s0 + p1 * s1 + p2 * s2 + p3 * s3;

    double t0 = pv0 * z00 + pv1 * z10 + pv2 * z20 + pv3 * z30;
    double t1 = pv0 * z01 + pv1 * z11 + pv2 * z21 + pv3 * z31;
    double t2 = pv0 * z02 + pv1 * z12 + pv2 * z22 + pv3 * z32;
    double t3 = pv0 * z03 + pv1 * z13 + pv2 * z23 + pv3 * z33;
    res.zy = b0 * t0 + b1 * t1 + b2 * t2 + b3 * t3;
    if (target != GF_IP_SECOND) return;

    res.zxy = pv0 * s0 + pv1 * s1 + pv2 * s2 + pv3 * s3;

    const double buu0 = bu.dd[0], buu1 = bu.dd[1], buu2 = bu.dd[2], buu3 = bu.dd[3];
    s0 = buu0 * z00 + buu1 * z01 + buu2 * z02 + buu3 * z03;
    s1 = buu0 * z10 + buu1 * z11 + buu2 * z12 + buu3 * z13;
    s2 = buu0 * z20 + buu1 * z21 + buu2 * z22 + buu3 * z23;
    s3 = buu0 * z30 + buu1 * z31 + buu2 * z32 + buu3 * z33;
    res.zxx = p0 * s0 + p1 * s1 + p2 * s2 + p3 * s3;

    const double pvv0 = pv.dd[0], pvv1 = pv.dd[1], pvv2 = pv.dd[2], pvv3 = pv.dd[3];
    t0 = pvv0 * z00 + pvv1 * z10 + pvv2 * z20 + pvv3 * z30;
    t1 = pvv0 * z01 + pvv1 * z11 + pvv2 * z21 + pvv3 * z31;
    t2 = pvv0 * z02 + pvv1 * z12 + pvv2 * z22 + pvv3 * z32;
    t3 = pvv0 * z03 + pvv1 * z13 + pvv2 * z23 + pvv3 * z33;
    res.zyy = b0 * t0 + b1 * t1 + b2 * t2 + b3 * t3;
}

// InterpolationResult.getUnitNormal (:129-139)
GF_HD void gf_interp_unit_normal(double zx, double zy, double *n)
{
    const double s = sqrt(zx * zx + zy * zy + 1);
    n[0] = -zx / s;
    n[1] = -zy / s;
    n[2] = 1.0 / s;
}

GF_HD void gf_interp_nullify(GfInterpResult &res)                               // InterpolationResult.java:141-151
{
    const double qnan = gf_interp_sample_f32(0x7fc00000u);
    res.z = res.zx = res.zy = res.zxx = res.zxy = res.zyy = qnan;
    res.normal[0] = res.normal[1] = res.normal[2] = qnan;
}

// One point: window, bounds, the spacing check (InterpolatorBSpline.java:304-307), the sixteen samples, evaluation; the unit normal
// only when wantNormal.  Everything is NaN unless the status is GF_IP_OK.
GF_HD int gf_interp_point(const GfInterpGeom &g, const void *block, double row, double col, double columnSpacing, bool wantNormal,
                       GfInterpResult &res)
{
    gf_interp_nullify(res);
    GfInterpWindow w;
    int status = gf_interp_window(g, row, col, w);
    if (status == GF_IP_OK && !gf_interp_window_in_block(g, w.row0, w.col0, w.n1)) status = GF_IP_ERR_BOUNDS;
    if (status == GF_IP_OK && g.target != GF_IP_VALUE && (columnSpacing == 0 || g.rowSpacing == 0)) status = GF_IP_ERR_ARG;
    if (status != GF_IP_OK) return status;
    double z[16];
    gf_interp_samples(g, block, w.row0, w.col0, w.n1, z);
    GfInterpBasis bu, pv;
    gf_interp_basis(w.u, columnSpacing, g.target, bu);
    gf_interp_basis(w.v, g.rowSpacing, g.target, pv);
    gf_interp_sums(z, bu, pv, g.target, res);
    if (wantNormal) gf_interp_unit_normal(res.zx, res.zy, res.normal);
    return GF_IP_OK;
}
